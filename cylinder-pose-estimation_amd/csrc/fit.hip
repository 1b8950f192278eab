// Geometric half of the hot path for gfx950: one wavefront (64 lanes) per stereo frame.
//   reference: utils/fitSingleCylinder.m:5-25, chooseIdx.m:19-104, findGridCorrespondences.m,
//   triangulateWithThreshold.m:16-43, fitCylinderWPts3.m, getDistPts3ToLine.m, estCurvatures.m,
//   fitplane.m, applyCylParamsPrior.m, cylParams2T.m; [ext] MATLAB triangulate / pca / knnsearch /
//   fminsearch restated as in SURVEY.md appendix B.
//
// Nothing here is a dense contraction (per-point 4x4 SVDs, per-frame reductions), so this is plain
// f64 VALU work, no MFMA.  Every reduction over the points of a frame is the fixed tree "lane l
// adds points l, l+64, ... in order, then xor-butterfly 32..1" and the build uses
// -ffp-contract=off, so results are bit-identical to the CPU oracle's.
//
// k_select_triangulate : index join through dense (col,row)->slot tables, per-point DLT
//                        triangulation (one lane per point), the 3x3 patch scan of chooseIdx with
//                        per-point errors reused across patches, compaction in the reference's
//                        output order (containers.Map string-key order).
// k_fit_cylinder       : mean / PCA / nearest-to-axis point / 20-NN quadric at that one point /
//                        Nelder-Mead (MATLAB fminsearch order) / applyCylParamsPrior / cylParams2T.
#include "cpe_internal.h"
#include <float.h>

namespace {

constexpr int MAXP = CPE_MAXP;
// the per-point LDS arrays of the one-wavefront-per-frame kernels (dynamic: they exceed the static 64 KB limit)
extern __shared__ double fit_dyn[];
constexpr size_t SEL_LDS_BYTES = (size_t)MAXP * (3 * 8 + 8 + 8 + 4 + 4 + 1);
constexpr size_t FIT_LDS_BYTES = (size_t)MAXP * 4 * 8;
constexpr size_t RANSAC_LDS_BYTES = (size_t)MAXP * 7 * 8;
constexpr int TBL = CPE_FIT_TABLE_DIM;  // dense (col,row) table is TBL x TBL per image
constexpr int MAXU = TBL;

__device__ __forceinline__ double wave_sum(double p)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    return p;
}
__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// P = K * T(1:3,:)
__device__ void make_P(const double *K, const double *T, double *P)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s = s + K[r * 3 + k] * T[k * 4 + c];
            P[r * 4 + c] = s;
        }
}

// one-sided Jacobi SVD of a 4x4, returns the right singular vector of the smallest singular value
__device__ void svd4_null(double *U, double *x)
{
    double V[16];
#pragma unroll
    for (int i = 0; i < 16; i++) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        int rotated = 0;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    al = al + U[k * 4 + p] * U[k * 4 + p];
                    be = be + U[k * 4 + q] * U[k * 4 + q];
                    ga = ga + U[k * 4 + p] * U[k * 4 + q];
                }
                if (!(fabs(ga) <= 1e-15 * sqrt(al * be))) {
                    rotated = 1;
                    double zeta = (be - al) / (2.0 * ga);
                    double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    if (zeta < 0) t = -t;
                    double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        double up = U[k * 4 + p], uq = U[k * 4 + q];
                        U[k * 4 + p] = c * up - s * uq;
                        U[k * 4 + q] = s * up + c * uq;
                        double vp = V[k * 4 + p], vq = V[k * 4 + q];
                        V[k * 4 + p] = c * vp - s * vq;
                        V[k * 4 + q] = s * vp + c * vq;
                    }
                }
            }
        if (!rotated) break;
    }
    double best = 0;
    x[0] = x[1] = x[2] = x[3] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double nn = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) nn = nn + U[k * 4 + j] * U[k * 4 + j];
        if (j == 0 || nn < best) {
            best = nn;
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = V[k * 4 + j];
        }
    }
}

__device__ __forceinline__ void project(const double *P, const double *X, double &u, double &v)
{
    double a = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    double b = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    double c = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    u = a / c;
    v = b / c;
}

__device__ void triangulate_one(const double *P1, const double *P2, double u1, double v1, double u2,
                                double v2, double *X, double &err)
{
    double A[16], x[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        A[0 * 4 + c] = u1 * P1[8 + c] - P1[c];
        A[1 * 4 + c] = v1 * P1[8 + c] - P1[4 + c];
        A[2 * 4 + c] = u2 * P2[8 + c] - P2[c];
        A[3 * 4 + c] = v2 * P2[8 + c] - P2[4 + c];
    }
    svd4_null(A, x);
    X[0] = x[0] / x[3];
    X[1] = x[1] / x[3];
    X[2] = x[2] / x[3];
    double u, v, dx, dy;
    project(P1, X, u, v);
    dx = u1 - u;
    dy = v1 - v;
    double e1 = sqrt(dx * dx + dy * dy);
    project(P2, X, u, v);
    dx = u2 - u;
    dy = v2 - v;
    double e2 = sqrt(dx * dx + dy * dy);
    err = (e1 + e2) / 2.0;
}

// order of the char keys sprintf('%d_%d', c, r) in a containers.Map (chooseIdx.m:69,89):
// strings compare by char code, '-' < digits < '_'; encoded base 13 (pad 0) into one integer.
__device__ unsigned long long string_key(int c, int r)
{
    int codes[12];
    int n = 0;
    int vals[2] = {c, r};
    for (int part = 0; part < 2; part++) {
        int v = vals[part];
        if (v < 0) { codes[n++] = 1; v = -v; }
        int dig[5], nd = 0;
        do { dig[nd++] = v % 10; v /= 10; } while (v > 0 && nd < 5);
        for (int k = nd - 1; k >= 0; k--) codes[n++] = 2 + dig[k];
        if (part == 0) codes[n++] = 12;
    }
    unsigned long long key = 0;
    for (int k = 0; k < 11; k++) key = key * 13ull + (unsigned long long)(k < n ? codes[k] : 0);
    return key;
}

__global__ __launch_bounds__(64) void k_select_triangulate(
    const double *__restrict__ xy1, const int *__restrict__ id1, const int *__restrict__ cnt1,
    const double *__restrict__ xy2, const int *__restrict__ id2, const int *__restrict__ cnt2,
    const double *__restrict__ K1, const double *__restrict__ K2, const double *__restrict__ T21,
    int selector, int patch, double th, int *__restrict__ tables /* n * 2 * TBL*TBL */,
    double *__restrict__ o_p1, double *__restrict__ o_p2, int *__restrict__ o_idx,
    double *__restrict__ o_X, double *__restrict__ o_err, int *__restrict__ o_m,
    double *__restrict__ o_mean_err, int *__restrict__ o_flags)
{
    __builtin_amdgcn_s_setprio(3);   // one wavefront per frame beside wide kernels (see k_fit_cylinder)
    // per-point arrays: dynamic LDS (SEL_LDS_BYTES; more than the 64 KB a kernel may declare statically)
    double *sX = fit_dyn;                                                                   // [MAXP * 3]
    double *sErr = sX + MAXP * 3;                                                           // [MAXP]
    unsigned long long *sKey = reinterpret_cast<unsigned long long *>(sErr + MAXP);         // [MAXP]
    int *sJ = reinterpret_cast<int *>(sKey + MAXP);                                         // [MAXP] matching slot in image 2 (or -1)
    int *sOrder = sJ + MAXP;                                                                // [MAXP] output position -> gp1 slot
    unsigned char *sSel = reinterpret_cast<unsigned char *>(sOrder + MAXP);                 // [MAXP]
    __shared__ int sUx[MAXU], sUy[MAXU];
    __shared__ unsigned char sFx[MAXU], sFy[MAXU];
    const int f = blockIdx.x, lane = threadIdx.x;
    const double *a1 = xy1 + (size_t)f * MAXP * 2, *a2 = xy2 + (size_t)f * MAXP * 2;
    const int *i1 = id1 + (size_t)f * MAXP * 2, *i2 = id2 + (size_t)f * MAXP * 2;
    int n1 = min(max(cnt1[f], 0), MAXP), n2 = min(max(cnt2[f], 0), MAXP);
    int *t1 = tables + (size_t)f * 2 * TBL * TBL, *t2 = t1 + TBL * TBL;
    int flags = 0;

    // index range over both tables
    int cmin = INT_MAX, cmax = INT_MIN, rmin = INT_MAX, rmax = INT_MIN;
    for (int i = lane; i < n1; i += 64) {
        int c = i1[2 * i], r = i1[2 * i + 1];
        cmin = min(cmin, c); cmax = max(cmax, c); rmin = min(rmin, r); rmax = max(rmax, r);
    }
    for (int i = lane; i < n2; i += 64) {
        int c = i2[2 * i], r = i2[2 * i + 1];
        cmin = min(cmin, c); cmax = max(cmax, c); rmin = min(rmin, r); rmax = max(rmax, r);
    }
    cmin = wave_min_i(cmin); cmax = wave_max_i(cmax); rmin = wave_min_i(rmin); rmax = wave_max_i(rmax);
    int m = 0;
    bool ok = n1 > 0 && n2 > 0;
    if (ok && ((long long)cmax - cmin >= TBL || (long long)rmax - rmin >= TBL || cmin < -9999 || cmax > 9999 ||
               rmin < -9999 || rmax > 9999)) {
        ok = false;
        flags |= CPE_FIT_FLAG_OVERFLOW;
    }
    if (ok) {
        const int tw = cmax - cmin + 1, thh = rmax - rmin + 1;
        for (int i = lane; i < tw * thh; i += 64) { t1[i] = INT_MAX; t2[i] = INT_MAX; }
        __syncthreads();
        for (int i = lane; i < n1; i += 64) atomicMin(&t1[(i1[2 * i + 1] - rmin) * tw + (i1[2 * i] - cmin)], i);
        for (int i = lane; i < n2; i += 64) atomicMin(&t2[(i2[2 * i + 1] - rmin) * tw + (i2[2 * i] - cmin)], i);
        __syncthreads();
#define TBL1(c, r) __hip_atomic_load(&t1[((r) - rmin) * tw + ((c) - cmin)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define TBL2(c, r) __hip_atomic_load(&t2[((r) - rmin) * tw + ((c) - cmin)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
        double P1[12], P2[12];
        {
            const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            double k1[9], k2[9], tt[16];
            for (int k = 0; k < 9; k++) { k1[k] = K1[k]; k2[k] = K2[k]; }
            for (int k = 0; k < 16; k++) tt[k] = T21[k];
            make_P(k1, I4, P1);
            make_P(k2, tt, P2);
        }
        // join (first occurrence on both sides) + per-point triangulation
        int njoin = 0;
        for (int i = lane; i < n1; i += 64) {
            int c = i1[2 * i], r = i1[2 * i + 1];
            int j = TBL2(c, r);
            int jj = (j != INT_MAX) ? j : -1;
            sJ[i] = jj;
            sSel[i] = 0;
            if (jj >= 0) {
                double X[3], e;
                triangulate_one(P1, P2, a1[2 * i], a1[2 * i + 1], a2[2 * jj], a2[2 * jj + 1], X, e);
                sX[3 * i] = X[0]; sX[3 * i + 1] = X[1]; sX[3 * i + 2] = X[2];
                sErr[i] = e;
                njoin++;
            }
        }
        njoin = wave_sum_i(njoin);
        __syncthreads();

        bool string_order = false;
        if (selector == 0 && njoin > 0) {
            // unique sorted col / row values of image 1 (chooseIdx.m:22-23)
            int nx = 0, ny = 0;
            for (int i = lane; i < MAXU; i += 64) { sFx[i] = 0; sFy[i] = 0; }
            __syncthreads();
            for (int i = lane; i < n1; i += 64) { sFx[i1[2 * i] - cmin] = 1; sFy[i1[2 * i + 1] - rmin] = 1; }
            __syncthreads();
            if (lane == 0) {
                for (int c = 0; c < tw; c++)
                    if (sFx[c]) sUx[nx++] = c + cmin;
                for (int r = 0; r < thh; r++)
                    if (sFy[r]) sUy[ny++] = r + rmin;
            }
            nx = __shfl(nx, 0, 64);
            ny = __shfl(ny, 0, 64);
            __syncthreads();
            const int px = nx - patch + 1, py = ny - patch + 1;
            int nsel = 0;
            if (px > 0 && py > 0) {
                for (int pidx = lane; pidx < px * py; pidx += 64) {
                    int ix = pidx / py, iy = pidx - ix * py;
                    bool all = true;
                    double s = 0.0;
                    for (int a = 0; a < patch && all; a++)
                        for (int b = 0; b < patch; b++) {
                            int c = sUx[ix + a], r = sUy[iy + b];
                            int s1 = TBL1(c, r), s2 = TBL2(c, r);
                            if (s1 == INT_MAX || s2 == INT_MAX) { all = false; break; }
                            s = s + sErr[s1];
                        }
                    if (all && (s / (double)(patch * patch) < th)) {
                        for (int a = 0; a < patch; a++)
                            for (int b = 0; b < patch; b++) sSel[TBL1(sUx[ix + a], sUy[iy + b])] = 1;
                    }
                }
            }
            __syncthreads();
            for (int i = lane; i < n1; i += 64) nsel += sSel[i];
            nsel = wave_sum_i(nsel);
            if (nsel > 0) string_order = true;
            else flags |= CPE_FIT_FLAG_FALLBACK;
        } else if (selector == 1 && njoin > 0) {
            int nsel = 0;
            for (int i = lane; i < n1; i += 64) {
                unsigned char sel = (sJ[i] >= 0 && sErr[i] < th) ? 1 : 0;
                sSel[i] = sel;
                nsel += sel;
            }
            nsel = wave_sum_i(nsel);
            if (nsel == 0) flags |= CPE_FIT_FLAG_FALLBACK;
        } else {
            flags |= (selector == 2) ? 0 : CPE_FIT_FLAG_FALLBACK;
        }
        __syncthreads();
        if ((flags & CPE_FIT_FLAG_FALLBACK) || selector == 2)
            for (int i = lane; i < n1; i += 64) sSel[i] = sJ[i] >= 0 ? 1 : 0;
        __syncthreads();

        // output order
        if (string_order) {
            for (int i = lane; i < n1; i += 64)
                sKey[i] = sSel[i] ? string_key(i1[2 * i], i1[2 * i + 1]) : ~0ull;
            __syncthreads();
            for (int i = lane; i < n1; i += 64) {
                if (!sSel[i]) continue;
                unsigned long long ki = sKey[i];
                int rank = 0;
                for (int j = 0; j < n1; j++) rank += (sKey[j] < ki) ? 1 : 0;
                sOrder[rank] = i;
            }
            for (int i = lane; i < n1; i += 64) m += sSel[i];
            m = wave_sum_i(m);
        } else {
            int base = 0;
            for (int i0 = 0; i0 < n1; i0 += 64) {
                int i = i0 + lane;
                bool sel = i < n1 && sSel[i];
                unsigned long long bal = __ballot(sel);
                if (sel) sOrder[base + __popcll(bal & ((1ull << lane) - 1ull))] = i;
                base += __popcll(bal);
            }
            m = base;
        }
        __syncthreads();
        double es = 0.0;
        for (int k = lane; k < m; k += 64) {
            int i = sOrder[k], j = sJ[i];
            size_t o = (size_t)f * MAXP + k;
            o_p1[2 * o] = a1[2 * i]; o_p1[2 * o + 1] = a1[2 * i + 1];
            o_p2[2 * o] = a2[2 * j]; o_p2[2 * o + 1] = a2[2 * j + 1];
            o_idx[2 * o] = i1[2 * i]; o_idx[2 * o + 1] = i1[2 * i + 1];
            o_X[3 * o] = sX[3 * i]; o_X[3 * o + 1] = sX[3 * i + 1]; o_X[3 * o + 2] = sX[3 * i + 2];
            o_err[o] = sErr[i];
            es = es + sErr[i];
        }
        es = wave_sum(es);
        if (lane == 0) o_mean_err[f] = m > 0 ? es / (double)m : 0.0;
#undef TBL1
#undef TBL2
    } else if (lane == 0) {
        o_mean_err[f] = 0.0;
    }
    if (lane == 0) { o_m[f] = m; o_flags[f] = flags; }
}

// ------------------------------------------------------------------------------------------ fit
struct Pts {
    const double *p;  // LDS, 3 per point
    int n;
};

// ---- the small dense algebra of the fits, once each.  Constant indices after unrolling throughout, so every matrix stays in
// registers (a run-time row index puts the whole matrix into scratch memory).

// the axis of a line given as origin o and direction d, as getDistPts3ToLine.m gets it: p2 = o + d, v = p2 - o.  The round trip
// is deliberate: it reproduces the reference's rounding.  A cylinder's 6-vector x is axis_of(x, x + 3, ...).
__device__ __forceinline__ void axis_of(const double *o, const double *d, double *v, double &nv2)
{
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = (o[k] + d[k]) - o[k];
    nv2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
}

// a point against the axis (org, v, nv2): al = ((pt - org).v)/|v|^2, e = (pt - org) - v al, dd = |e| (getDistPts3ToLine.m)
__device__ __forceinline__ void point_on_axis(const double *pt, const double *org, const double *v, double nv2, double &al, double *e,
                                              double &dd)
{
    al = (((pt[0] - org[0]) * v[0] + (pt[1] - org[1]) * v[1]) + (pt[2] - org[2]) * v[2]) / nv2;
#pragma unroll
    for (int k = 0; k < 3; k++) e[k] = pt[k] - (org[k] + v[k] * al);
    dd = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

__device__ __forceinline__ double dist_pt_line(const double *x, const double *p1, const double *v, double nv2)
{
    double al, e[3], dd;
    point_on_axis(x, p1, v, nv2, al, e, dd);
    return dd;
}

// dist() of fitCylinderWPts3.m:44-49
__device__ double cyl_objective(const double *x, const Pts &P, double R, int lane)
{
    double v[3], nv2;
    axis_of(x, x + 3, v, nv2);
    double acc = 0.0;
    for (int k = lane; k < P.n; k += 64) {
        double d = dist_pt_line(P.p + 3 * k, x, v, nv2);
        double w = d - R;
        acc = acc + w * w;
    }
    return wave_sum(acc);
}

// one row j[N] of a Jacobian with its residual r into acc: the upper triangle of J'J packed by rows (N (N + 1) / 2 sums), then J'r (N)
template <int N>
__device__ __forceinline__ void normal_accumulate(const double *j, double r, double *acc)
{
    int i = 0;
#pragma unroll
    for (int a = 0; a < N; a++) {
#pragma unroll
        for (int b = a; b < N; b++) { acc[i] = acc[i] + j[a] * j[b]; i++; }
        acc[N * (N + 1) / 2 + a] = acc[N * (N + 1) / 2 + a] + j[a] * r;
    }
}

// M x = b for NRHS right-hand sides by Gaussian elimination with partial pivoting, in place: M row-major N x N, b and x row-major
// N x NRHS.  The pivot of a column is the first row of the largest |.|; row swaps are conditional swaps.  false: a zero pivot
// (the arithmetic is finished all the same; the caller discards x).
template <int N, int NRHS = 1>
__device__ __forceinline__ bool gauss_solve(double *M, double *b, double *x)
{
    bool singular = false;
#pragma unroll
    for (int c = 0; c < N; c++) {
        int pv = c;
        double best = fabs(M[c * N + c]);
#pragma unroll
        for (int r = c + 1; r < N; r++) {
            const double av = fabs(M[r * N + c]);
            if (av > best) { best = av; pv = r; }
        }
#pragma unroll
        for (int r = c + 1; r < N; r++) {
            const bool sw = pv == r;   // selects of values, not a branch: a branch becomes a choice between row addresses
#pragma unroll
            for (int k = 0; k < N; k++) { const double mc = M[c * N + k], mr = M[r * N + k]; M[c * N + k] = sw ? mr : mc; M[r * N + k] = sw ? mc : mr; }
#pragma unroll
            for (int k = 0; k < NRHS; k++) { const double bc = b[c * NRHS + k], br = b[r * NRHS + k]; b[c * NRHS + k] = sw ? br : bc; b[r * NRHS + k] = sw ? bc : br; }
        }
        singular = singular || M[c * N + c] == 0;
#pragma unroll
        for (int r = c + 1; r < N; r++) {
            const double fct = M[r * N + c] / M[c * N + c];
#pragma unroll
            for (int k = c; k < N; k++) M[r * N + k] = M[r * N + k] - fct * M[c * N + k];
#pragma unroll
            for (int k = 0; k < NRHS; k++) b[r * NRHS + k] = b[r * NRHS + k] - fct * b[c * NRHS + k];
        }
    }
#pragma unroll
    for (int j = 0; j < NRHS; j++)
#pragma unroll
        for (int r = N - 1; r >= 0; r--) {
            double s = b[r * NRHS + j];
#pragma unroll
            for (int k = r + 1; k < N; k++) s = s - M[r * N + k] * x[k * NRHS + j];
            x[r * NRHS + j] = s / M[r * N + r];
        }
    return !singular;
}

// eigenvectors of a symmetric N x N by cyclic Jacobi rotations, p < q by rows, at most 30 sweeps: V's columns, w unsorted
template <int N>
__device__ __forceinline__ void jacobi_eig(const double *Ain, double *w, double *V)
{
    double A[N * N];
#pragma unroll
    for (int i = 0; i < N * N; i++) { A[i] = Ain[i]; V[i] = (i % (N + 1) == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; sweep++) {
        int rotated = 0;
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p * N + q];
                if (!(fabs(apq) <= 1e-17 * (fabs(A[p * N + p]) + fabs(A[q * N + q])))) {
                    rotated = 1;
                    const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0) t = -t;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        const double akp = A[k * N + p], akq = A[k * N + q];
                        A[k * N + p] = c * akp - s * akq;
                        A[k * N + q] = s * akp + c * akq;
                    }
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        const double apk = A[p * N + k], aqk = A[q * N + k];
                        A[p * N + k] = c * apk - s * aqk;
                        A[q * N + k] = s * apk + c * aqk;
                    }
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        const double vkp = V[k * N + p], vkq = V[k * N + q];
                        V[k * N + p] = c * vkp - s * vkq;
                        V[k * N + q] = s * vkp + c * vkq;
                    }
                }
            }
        if (!rotated) break;
    }
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = A[i * (N + 1)];
}

// jacobi_eig<3> with the eigenvalues ascending: a stable bubble over the columns (as the oracle)
__device__ void eig3(const double *Ain, double *w, double *V)
{
    jacobi_eig<3>(Ain, w, V);
    auto cswap = [&](int a, int b) {
        if (!(w[b] < w[a])) return;
        const double t_ = w[a]; w[a] = w[b]; w[b] = t_;
#pragma unroll
        for (int k = 0; k < 3; k++) { const double u_ = V[k * 3 + a]; V[k * 3 + a] = V[k * 3 + b]; V[k * 3 + b] = u_; }
    };
    cswap(0, 1); cswap(1, 2); cswap(0, 1);
}

__device__ __forceinline__ double eps_of(double x)  // MATLAB eps(x)
{
    x = fabs(x);
    if (x < DBL_MIN) return 4.9406564584124654e-324;
    int e;
    frexp(x, &e);
    return ldexp(1.0, e - 53);
}

// ---- the pieces of fitCylinderWPts3.m as device functions (one wavefront, points in LDS); k_fit_cylinder runs them on
// all points of a frame, k_fit_ransac (build-defined, BASELINE config 5) on subsets as well
// initial cylinder (fitCylinderWPts3.m:7-36): x0 = [origin, direction], f0 = objective at x0
__device__ void fit_init(const double *sP, int n, double R, int lane, double *sD, int *sNb, double *x0, double &f0_out)
{
    Pts P{sP, n};
    // ctr = mean(Pts3,2); covariance; rdir = pca 3rd axis with z > 0 (fitCylinderWPts3.m:7-19)
    double ctr[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double acc = 0.0;
        for (int k = lane; k < n; k += 64) acc = acc + sP[3 * k + c];
        ctr[c] = wave_sum(acc) / (double)n;
    }
    double Cv[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++) {
            double acc = 0.0;
            for (int k = lane; k < n; k += 64) acc = acc + (sP[3 * k + a] - ctr[a]) * (sP[3 * k + b] - ctr[b]);
            double v = wave_sum(acc) / (double)(n - 1);
            Cv[a * 3 + b] = v;
            Cv[b * 3 + a] = v;
        }
    double w3[3], V3[9];
    eig3(Cv, w3, V3);
    double rdir[3] = {V3[0], V3[3], V3[6]};
    if (rdir[2] < 0) { rdir[0] = -rdir[0]; rdir[1] = -rdir[1]; rdir[2] = -rdir[2]; }

    // i = argmin dist to line(ctr, ctr + rdir)  (first minimum)
    int im;
    {
        double v[3], nv2;
        axis_of(ctr, rdir, v, nv2);
        double bd = DBL_MAX;
        int bi = INT_MAX;
        for (int k = lane; k < n; k += 64) {
            double d = dist_pt_line(sP + 3 * k, ctr, v, nv2);
            if (d < bd) { bd = d; bi = k; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            double od = __shfl_xor(bd, off, 64);
            int oi = __shfl_xor(bi, off, 64);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        im = bi;
    }
    double e0 = ctr[0] - sP[3 * im], e1 = ctr[1] - sP[3 * im + 1], e2 = ctr[2] - sP[3 * im + 2];
    double d2s = sqrt((e0 * e0 + e1 * e1) + e2 * e2);

    // estCurvatures at point im only: 20-NN (ties by index), plane, local frame, quadric, 2x2 eig
    const int K = n < 20 ? n : 20;
    for (int k = lane; k < n; k += 64) {
        double a = sP[3 * k] - sP[3 * im], b = sP[3 * k + 1] - sP[3 * im + 1], c = sP[3 * k + 2] - sP[3 * im + 2];
        sD[k] = (a * a + b * b) + c * c;
    }
    __syncthreads();
    for (int r = 0; r < K; r++) {
        double bd = DBL_MAX;
        int bi = INT_MAX;
        for (int k = lane; k < n; k += 64) {
            double d = sD[k];
            if (d >= 0 && d < bd) { bd = d; bi = k; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            double od = __shfl_xor(bd, off, 64);
            int oi = __shfl_xor(bi, off, 64);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        if (lane == 0) { sNb[r] = bi; sD[bi] = -1.0; }
        __syncthreads();
    }
    double dir0[3];
    {
        double mu[3] = {0, 0, 0};
        for (int k = 0; k < K; k++)
            for (int c = 0; c < 3; c++) mu[c] = mu[c] + sP[3 * sNb[k] + c];
        for (int c = 0; c < 3; c++) mu[c] = mu[c] / (double)K;
        double C2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < K; k++) {
            double e[3] = {sP[3 * sNb[k]] - mu[0], sP[3 * sNb[k] + 1] - mu[1], sP[3 * sNb[k] + 2] - mu[2]};
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) C2[a * 3 + b] = C2[a * 3 + b] + e[a] * e[b];
        }
#pragma unroll
        for (int a = 0; a < 9; a++) C2[a] = C2[a] / (double)(K - 1);
        double w[3], V[9];
        eig3(C2, w, V);
        double z[3] = {V[0], V[3], V[6]};
        if (z[2] < 0) { z[0] = -z[0]; z[1] = -z[1]; z[2] = -z[2]; }  // normal away from the camera (documented)
        double x[3] = {1, 0, 0};
        if (fabs(z[0]) > 0.9) { x[0] = 0; x[1] = 1; }
        double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
        double xx[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
        double M[25], rhs[5], co[5];
        for (int a = 0; a < 25; a++) M[a] = 0;
        for (int a = 0; a < 5; a++) rhs[a] = 0;
        for (int k = 0; k < K; k++) {
            double e[3] = {sP[3 * sNb[k]] - mu[0], sP[3 * sNb[k] + 1] - mu[1], sP[3 * sNb[k] + 2] - mu[2]};
            double lx = (e[0] * xx[0] + e[1] * xx[1]) + e[2] * xx[2];
            double ly = (e[0] * y[0] + e[1] * y[1]) + e[2] * y[2];
            double lz = (e[0] * z[0] + e[1] * z[1]) + e[2] * z[2];
            double row[5] = {lx * lx, lx * ly, ly * ly, lx, ly};
            for (int a = 0; a < 5; a++) {
                for (int b = 0; b < 5; b++) M[a * 5 + b] = M[a * 5 + b] + row[a] * row[b];
                rhs[a] = rhs[a] + row[a] * lz;
            }
        }
        gauss_solve<5>(M, rhs, co);
        double a = co[0] * 2, b = co[1], c = co[2] * 2;
        double hd = (a - c) / 2.0, mid = (a + c) / 2.0, rad = sqrt(hd * hd + b * b);
        double lam = mid - rad;  // eig ascending: V(:,1)
        double v0, v1;
        if (fabs(lam - a) >= fabs(lam - c)) { v0 = b; v1 = lam - a; }
        else { v0 = lam - c; v1 = b; }
        double nn = sqrt(v0 * v0 + v1 * v1);
        if (nn == 0) { v0 = 1; v1 = 0; nn = 1; }
        v0 = v0 / nn;
        v1 = v1 / nn;
        for (int k = 0; k < 3; k++) dir0[k] = xx[k] * v0 + y[k] * v1;
    }

#pragma unroll
    for (int c = 0; c < 3; c++) {
        x0[c] = ctr[c] + rdir[c] * (R - d2s);
        x0[3 + c] = dir0[c];
    }
    f0_out = cyl_objective(x0, P, R, lane);
}

// the objective of the per-frame fit as fit_nm_on takes it
struct CylObjective {
    Pts P;
    double R;
    int lane;
    __device__ double operator()(const double *x) const { return cyl_objective(x, P, R, lane); }
};

// fminsearch (MATLAB order) from x0 on any objective `double obj(const double *x)` (wave-uniform result); one body for the
// per-frame fit (CylObjective) and the multi-frame fit (MultiObjective, which holds workgroup barriers: every wave of its
// workgroup runs this loop on the same numbers, so all of them call obj the same number of times)
template <class Obj>
__device__ __forceinline__ void fit_nm_on(Obj &obj, double tolx, double tolf, int maxiter, int maxfun, const double *x0, double f0,
                                          double *xf, double &ffinal, int &itercount, int &func_evals)
{
    // ---- fminsearch (MATLAB order).  simplex is wave-uniform, kept in registers.
    constexpr int N = 6;
    double v[N + 1][N], fv[N + 1];
#pragma unroll
    for (int k = 0; k < N; k++) v[0][k] = x0[k];
    fv[0] = f0;
#pragma unroll
    for (int j = 0; j < N; j++) {
#pragma unroll
        for (int k = 0; k < N; k++) v[j + 1][k] = x0[k];
        if (v[j + 1][j] != 0) v[j + 1][j] = (1 + 0.05) * v[j + 1][j];
        else v[j + 1][j] = 0.00025;
        fv[j + 1] = obj(v[j + 1]);
    }
    func_evals = N + 1;
    itercount = 1;
#define CSWAPV(a)                                                                       \
    if (fv[a] > fv[a + 1]) {                                                            \
        double t_ = fv[a]; fv[a] = fv[a + 1]; fv[a + 1] = t_;                           \
        _Pragma("unroll") for (int k = 0; k < N; k++) { double u_ = v[a][k]; v[a][k] = v[a + 1][k]; v[a + 1][k] = u_; } \
    }
#define SORT_SIMPLEX()                                                                  \
    CSWAPV(0)                                                                           \
    CSWAPV(1) CSWAPV(0)                                                                 \
    CSWAPV(2) CSWAPV(1) CSWAPV(0)                                                       \
    CSWAPV(3) CSWAPV(2) CSWAPV(1) CSWAPV(0)                                             \
    CSWAPV(4) CSWAPV(3) CSWAPV(2) CSWAPV(1) CSWAPV(0)                                   \
    CSWAPV(5) CSWAPV(4) CSWAPV(3) CSWAPV(2) CSWAPV(1) CSWAPV(0)
    SORT_SIMPLEX()
    while (func_evals < maxfun && itercount < maxiter) {
        double df = 0, dx = 0, vmax = v[0][0];
#pragma unroll
        for (int j = 1; j <= N; j++) {
            double a = fabs(fv[0] - fv[j]);
            if (a > df) df = a;
#pragma unroll
            for (int k = 0; k < N; k++) {
                double b = fabs(v[j][k] - v[0][k]);
                if (b > dx) dx = b;
            }
        }
#pragma unroll
        for (int k = 1; k < N; k++)
            if (v[0][k] > vmax) vmax = v[0][k];
        double tf = 10 * eps_of(fv[0]), tx = 10 * eps_of(vmax);
        if (df <= (tolf > tf ? tolf : tf) && dx <= (tolx > tx ? tolx : tx)) break;

        double xbar[N], xr[N], xt[N];
#pragma unroll
        for (int k = 0; k < N; k++) {
            double s = v[0][k];
#pragma unroll
            for (int j = 1; j < N; j++) s = s + v[j][k];
            xbar[k] = s / (double)N;
        }
#pragma unroll
        for (int k = 0; k < N; k++) xr[k] = 2.0 * xbar[k] - 1.0 * v[N][k];
        double fxr = obj(xr);
        func_evals++;
        bool shrink = false;
        if (fxr < fv[0]) {
#pragma unroll
            for (int k = 0; k < N; k++) xt[k] = 3.0 * xbar[k] - 2.0 * v[N][k];
            double fxe = obj(xt);
            func_evals++;
            if (fxe < fxr) {
#pragma unroll
                for (int k = 0; k < N; k++) v[N][k] = xt[k];
                fv[N] = fxe;
            } else {
#pragma unroll
                for (int k = 0; k < N; k++) v[N][k] = xr[k];
                fv[N] = fxr;
            }
        } else if (fxr < fv[N - 1]) {
#pragma unroll
            for (int k = 0; k < N; k++) v[N][k] = xr[k];
            fv[N] = fxr;
        } else if (fxr < fv[N]) {
#pragma unroll
            for (int k = 0; k < N; k++) xt[k] = 1.5 * xbar[k] - 0.5 * v[N][k];
            double fxc = obj(xt);
            func_evals++;
            if (fxc <= fxr) {
#pragma unroll
                for (int k = 0; k < N; k++) v[N][k] = xt[k];
                fv[N] = fxc;
            } else shrink = true;
        } else {
#pragma unroll
            for (int k = 0; k < N; k++) xt[k] = 0.5 * xbar[k] + 0.5 * v[N][k];
            double fxcc = obj(xt);
            func_evals++;
            if (fxcc < fv[N]) {
#pragma unroll
                for (int k = 0; k < N; k++) v[N][k] = xt[k];
                fv[N] = fxcc;
            } else shrink = true;
        }
        if (shrink) {
#pragma unroll
            for (int j = 1; j <= N; j++) {
#pragma unroll
                for (int k = 0; k < N; k++) v[j][k] = v[0][k] + 0.5 * (v[j][k] - v[0][k]);
                fv[j] = obj(v[j]);
            }
            func_evals += N;
        }
        SORT_SIMPLEX()
        itercount++;
    }
#undef SORT_SIMPLEX
#undef CSWAPV

#pragma unroll
    for (int k = 0; k < 6; k++) xf[k] = v[0][k];
    ffinal = fv[0];
}

// the per-frame fit: fminsearch on dist() of fitCylinderWPts3.m:44-49
__device__ void fit_nm(const double *sP, int n, double R, int lane, double tolx, double tolf, int maxiter, int maxfun,
                       const double *x0, double f0, double *xf, double &ffinal, int &itercount, int &func_evals)
{
    CylObjective obj{Pts{sP, n}, R, lane};
    fit_nm_on(obj, tolx, tolf, maxiter, maxfun, x0, f0, xf, ffinal, itercount, func_evals);
}

// the damped system of a Levenberg-Marquardt trial: M = J'J (A: its upper triangle packed by rows) with M_aa (1 + lambda) +
// 1e-12 trace on the diagonal, M dl = -g.  false: singular
template <int N>
__device__ __forceinline__ bool lm_damped_solve(const double *A, const double *g, double lambda, double *dl)
{
    double M[N * N], rhs[N];
    int i = 0;
    double trA = 0;
#pragma unroll
    for (int a = 0; a < N; a++)
#pragma unroll
        for (int b = a; b < N; b++) { M[a * N + b] = A[i]; M[b * N + a] = A[i]; if (a == b) trA = trA + A[i]; i++; }
#pragma unroll
    for (int a = 0; a < N; a++) { M[a * N + a] = M[a * N + a] + lambda * M[a * N + a] + 1e-12 * trA; rhs[a] = -g[a]; }
    return gauss_solve<N>(M, rhs, dl);
}

// N = 2 in closed form (A = s00 s01 s11): elimination would give other bits
template <>
__device__ __forceinline__ bool lm_damped_solve<2>(const double *A, const double *g, double lambda, double *dl)
{
    const double trA = A[0] + A[2];
    const double m00 = A[0] + lambda * A[0] + 1e-12 * trA, m11 = A[2] + lambda * A[2] + 1e-12 * trA;
    const double det = m00 * m11 - A[1] * A[1];
    dl[0] = (A[1] * g[1] - m11 * g[0]) / det;
    dl[1] = (A[1] * g[0] - m00 * g[1]) / det;
    return det != 0;
}

// Levenberg-Marquardt from (x0, f0 = problem(x0)) on N unknowns: the one loop of the cylinder fit and the multi-frame pose fit
// (k_frame_angles_lm has the same loop written out, see there).  A problem supplies
//   normal(x, A, g)           one Jacobian pass at the current point x: J'J (upper triangle packed by rows) and J'r
//   bool candidate(x, dl, xn) the retraction xn of the step dl from x; false: xn may not be evaluated
//   double operator()(xn)     the objective
// lambda starts at 1e-3, x 10 on a rejected trial, / 10 (floor 1e-12) on an accepted one; at most 12 trials per iteration and
// min(maxiter, 200) iterations; stop when an iteration improves f by no more than tolf 1e-3 (1 + f) with a step of at most tolx,
// or when none of its trials is accepted.
//   - A singular system or an invalid candidate is a rejected trial: lambda x 10, it counts towards the 12, the objective is not
//     evaluated and func_evals stays.
//   - A NaN objective is a rejected trial (fn < fx is false), so every loop is bounded whatever the objective returns.
//   - func_evals comes in as what the caller has spent already (f0, and whatever chose x0) and counts every evaluation here.
//   - Barriers: the multi-frame problem's objective and normal() hold __syncthreads().  Every wave of its workgroup runs this
//     loop on the same numbers (frame list, terms and the sums come from LDS, everything else each wave computes for itself, and
//     the arithmetic is deterministic), so every branch here goes the same way in all waves.  Keep it so: no branch in this
//     loop may depend on the wave or the lane.
//   - NX numbers describe a point and N <= NX a step (the projector model keeps unit vectors whole in x and steps in their
//     tangent planes); NX = N everywhere else.
template <int N, int NX = N, class Problem>
__device__ __forceinline__ void lm_minimize(Problem &prob, const double *x0, double f0, double tolx, double tolf, int maxiter, double *x,
                                            double &fx, int &itercount, int &func_evals)
{
#pragma unroll
    for (int k = 0; k < NX; k++) x[k] = x0[k];
    fx = f0;
    double lambda = 1e-3;
    itercount = 0;
    for (; itercount < maxiter && itercount < 200;) {
        double A[N * (N + 1) / 2], g[N];
        prob.normal(x, A, g);
        itercount++;
        bool accepted = false;
        double dmax = 0;
        const double fprev = fx;
        for (int tr = 0; tr < 12 && !accepted; tr++) {
            double dl[N], xn[NX];
            if (!lm_damped_solve<N>(A, g, lambda, dl) || !prob.candidate(x, dl, xn)) { lambda = lambda * 10; continue; }
            const double fn = prob(xn);
            func_evals++;
            if (fn < fx) {
                dmax = 0;
#pragma unroll
                for (int k = 0; k < N; k++) dmax = fmax(dmax, fabs(dl[k]));
#pragma unroll
                for (int k = 0; k < NX; k++) x[k] = xn[k];
                fx = fn;
                lambda = fmax(lambda / 10, 1e-12);
                accepted = true;
            } else {
                lambda = lambda * 10;
            }
        }
        if (!accepted) break;
        if ((fprev - fx) <= tolf * 1e-3 * (1.0 + fx) && dmax <= tolx) break;
    }
}

// Levenberg-Marquardt on the per-frame objective (north_star's "Gauss-Newton/LM inner loop"; NOT what the reference runs --
// fitCylinderWPts3.m:38 uses fminsearch -- validated against the Nelder-Mead result).
// r_i = d_i - R;  dr/do = -e/d;  dr/dv = -(alpha/d) e  with  e = (P-o) - v alpha, alpha = ((P-o).v)/|v|^2.
// The 6-parameter form has two gauge directions (origin along the axis, |v|): the damping term handles them.
struct CylProblem : CylObjective {
    __device__ __forceinline__ void normal(const double *x, double *A, double *g) const
    {
        double acc[27], v[3], nv2;
#pragma unroll
        for (int k = 0; k < 27; k++) acc[k] = 0.0;
        axis_of(x, x + 3, v, nv2);
        for (int k = lane; k < P.n; k += 64) {
            double al, e[3], dd;
            point_on_axis(P.p + 3 * k, x, v, nv2, al, e, dd);
            if (dd > 0) {
                const double r = dd - R, c1 = -1.0 / dd, c2 = -(al / dd);
                const double j[6] = {c1 * e[0], c1 * e[1], c1 * e[2], c2 * e[0], c2 * e[1], c2 * e[2]};
                normal_accumulate<6>(j, r, acc);
            }
        }
#pragma unroll
        for (int k = 0; k < 21; k++) A[k] = wave_sum(acc[k]);
#pragma unroll
        for (int k = 0; k < 6; k++) g[k] = wave_sum(acc[21 + k]);
    }
    __device__ __forceinline__ bool candidate(const double *x, const double *dl, double *xn) const
    {
#pragma unroll
        for (int k = 0; k < 6; k++) xn[k] = x[k] + dl[k];
        return true;
    }
};

__device__ void fit_lm(const double *sP, int n, double R, int lane, double tolx, double tolf, int maxiter,
                       const double *x0, double f0, double *xf, double &ffinal, int &itercount, int &func_evals)
{
    CylProblem prob{{Pts{sP, n}, R, lane}};
    func_evals = 1;
    lm_minimize<6>(prob, x0, f0, tolx, tolf, maxiter, xf, ffinal, itercount, func_evals);
}

// the outputs of the per-frame fit and of RANSAC around it, per frame f
struct FitOut {
    double *raw, *cyl, *T, *fvals;
    int *iters, *status;
    // a frame that is not fitted: its status, every other output zero
    __device__ void write_failed(int f, int lane, int st) const
    {
        if (lane != 0) return;
        status[f] = st;
        iters[2 * f] = 0; iters[2 * f + 1] = 0;
        fvals[2 * f] = 0; fvals[2 * f + 1] = 0;
        for (int k = 0; k < 12; k++) { raw[12 * f + k] = 0; cyl[12 * f + k] = 0; }
        for (int k = 0; k < 16; k++) T[16 * f + k] = 0;
    }
    // applyCylParamsPrior.m on both rows (ymin over the n points given), cylParams2T.m on the final row
    __device__ void write_ok(int f, int lane, const double *sP, int n, const double *x0, const double *xf, double f0, double ffinal,
                             int itercount, int func_evals) const;
};

__device__ void FitOut::write_ok(int f, int lane, const double *sP, int n, const double *x0, const double *xf, double f0, double ffinal,
                                 int itercount, int func_evals) const
{
    // applyCylParamsPrior.m on both rows, cylParams2T.m on the final row
    double ymin = DBL_MAX;
    for (int k = lane; k < n; k += 64) ymin = fmin(ymin, sP[3 * k + 1]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ymin = fmin(ymin, __shfl_xor(ymin, off, 64));
    if (lane == 0) {
        double rows[2][6];
        for (int k = 0; k < 6; k++) { rows[0][k] = x0[k]; rows[1][k] = xf[k]; }
        for (int rI = 0; rI < 2; rI++) {
            for (int k = 0; k < 6; k++) raw[12 * f + 6 * rI + k] = rows[rI][k];
            double o[3] = {rows[rI][0], rows[rI][1], rows[rI][2]}, d[3] = {rows[rI][3], rows[rI][4], rows[rI][5]};
            if (d[1] < 0) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; }
            double t = 0;
            if (!(fabs(d[1]) < DBL_EPSILON)) t = (ymin - o[1]) / d[1];
            for (int c = 0; c < 3; c++) { rows[rI][c] = o[c] + t * d[c]; rows[rI][3 + c] = d[c]; }
            for (int k = 0; k < 6; k++) cyl[12 * f + 6 * rI + k] = rows[rI][k];
        }
        const double *cy = rows[1];
        double y[3] = {cy[3], cy[4], cy[5]};
        double ny = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
        for (int c = 0; c < 3; c++) y[c] = y[c] / ny;
        double z[3] = {0 * y[2] - 0 * y[1], 0 * y[0] - 1 * y[2], 1 * y[1] - 0 * y[0]};
        double nz = sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
        for (int c = 0; c < 3; c++) z[c] = z[c] / nz;
        double xv[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
        double nx = sqrt((xv[0] * xv[0] + xv[1] * xv[1]) + xv[2] * xv[2]);
        for (int c = 0; c < 3; c++) xv[c] = xv[c] / nx;
        double *Tf = T + 16 * f;
        for (int r = 0; r < 3; r++) { Tf[r * 4] = xv[r]; Tf[r * 4 + 1] = y[r]; Tf[r * 4 + 2] = z[r]; Tf[r * 4 + 3] = cy[r]; }
        Tf[12] = 0; Tf[13] = 0; Tf[14] = 0; Tf[15] = 1;
        fvals[2 * f] = f0;
        fvals[2 * f + 1] = ffinal;
        iters[2 * f] = itercount;
        iters[2 * f + 1] = func_evals;
        status[f] = CPE_ST_OK;
    }
}

// a cylinder worth status 0: every parameter and the objective finite (x, f are wave-uniform)
__device__ __forceinline__ bool fit_finite(const double *x, double f)
{
    bool ok = isfinite(f);
#pragma unroll
    for (int k = 0; k < 6; k++) ok = ok && isfinite(x[k]);
    return ok;
}

template <int MODE>
__global__ __launch_bounds__(64) void k_fit_cylinder(const double *__restrict__ X, const int *__restrict__ cnt,
                                                     double R, double tolx, double tolf, int maxiter,
                                                     int maxfun, const FitOut out)
{
    // One wavefront per frame, a chain of dependent f64 operations 200-300 simplex iterations long: beside the wide kernels of
    // the other chunk in flight it waited its turn at every instruction (2.2 ms alone, 12 ms in the overlapped trace).  Its
    // few waves ask for the highest issue priority of their SIMD; the wide kernels fill what is left (2.2 ms again in the
    // overlapped trace; the bench rate does not move -- A/B on one box: 3166 / 3199 / 3198 with, 3175 / 3203 / 3182 without --,
    // the latency of a chunk does).  The same on the other narrow kernels of the chain changed nothing measurable and was dropped.
    __builtin_amdgcn_s_setprio(3);
    double *sP = fit_dyn, *sD = fit_dyn + MAXP * 3;   // dynamic LDS, FIT_LDS_BYTES
    __shared__ int sNb[20];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(cnt[f], 0), MAXP);
    if (n < CPE_FIT_MIN_POINTS) { out.write_failed(f, lane, CPE_ST_FEW_POINTS); return; }
    const double *Xf = X + (size_t)f * MAXP * 3;
    for (int i = lane; i < 3 * n; i += 64) sP[i] = Xf[i];
    __syncthreads();
    double x0[6], f0, xf[6], ffinal;
    int itercount, func_evals;
    fit_init(sP, n, R, lane, sD, sNb, x0, f0);
    if (!fit_finite(x0, f0)) { out.write_failed(f, lane, CPE_ST_FEW_POINTS); return; }
    if constexpr (MODE == 0) fit_nm(sP, n, R, lane, tolx, tolf, maxiter, maxfun, x0, f0, xf, ffinal, itercount, func_evals);
    else fit_lm(sP, n, R, lane, tolx, tolf, maxiter, x0, f0, xf, ffinal, itercount, func_evals);
    if (!fit_finite(xf, ffinal)) { out.write_failed(f, lane, CPE_ST_FEW_POINTS); return; }
    out.write_ok(f, lane, sP, n, x0, xf, f0, ffinal, itercount, func_evals);
}

// ---- BUILD-DEFINED (BASELINE config 5; nothing like it in the reference): RANSAC around the fit -------
// H hypotheses per frame, one wavefront per frame.  Hypothesis 0 uses all points; hypothesis h > 0 keeps point k with
// probability S/n, decided by a counter-based hash of (seed, frame, h, k), so every lane decides for its own points and the
// subset does not depend on any sequential generator state.  A hypothesis = `hyp_iters` LM iterations on its subset
// (compacted into LDS in point order) from the all-points initial cylinder, scored by the number of points with
// | dist(point, axis) - R | < tau over ALL points; the first hypothesis with the largest count wins and the final fit
// (Nelder-Mead or LM) runs on its inliers.  Same arithmetic, same order as oracle/src/orc_fit.c:orc_fit_cylinder_ransac.
__device__ __forceinline__ unsigned long long ransac_hash(unsigned long long seed, unsigned long long frame, unsigned long long h,
                                                          unsigned long long k)
{
    unsigned long long z = (seed ^ (frame * 0xD1B54A32D192ED03ULL) ^ (h << 32) ^ k) + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// |dist - R| < tau for point k of sP under the cylinder x
__device__ __forceinline__ bool ransac_inlier(const double *sP, int k, const double *x, double R, double tau)
{
    double v[3], nv2;
    axis_of(x, x + 3, v, nv2);
    return fabs(dist_pt_line(sP + 3 * k, x, v, nv2) - R) < tau;
}

template <int MODE>
__global__ __launch_bounds__(64) void k_fit_ransac(const double *__restrict__ X, const int *__restrict__ cnt, double R, int H, int S,
                                                   double tau, unsigned long long seed, unsigned long long frame0, int hyp_iters,
                                                   double tolx, double tolf, int maxiter, int maxfun,
                                                   const FitOut out, int *__restrict__ o_ninl, uint8_t *__restrict__ o_mask)
{
    double *sP = fit_dyn, *sQ = fit_dyn + MAXP * 3, *sD = fit_dyn + MAXP * 6;   // dynamic LDS, RANSAC_LDS_BYTES
    __shared__ int sNb[20];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(cnt[f], 0), MAXP);
    uint8_t *mk = o_mask + (size_t)f * MAXP;
    for (int k = lane; k < MAXP; k += 64) mk[k] = 0;
    auto few_points = [&]() {   // status 5, zero outputs, empty mask
        out.write_failed(f, lane, CPE_ST_FEW_POINTS);
        if (lane == 0) o_ninl[f] = 0;
    };
    if (n < CPE_FIT_MIN_POINTS) { few_points(); return; }
    const double *Xf = X + (size_t)f * MAXP * 3;
    for (int i = lane; i < 3 * n; i += 64) sP[i] = Xf[i];
    __syncthreads();
    double x0[6], f0;
    fit_init(sP, n, R, lane, sD, sNb, x0, f0);
    if (!fit_finite(x0, f0)) { few_points(); return; }
    const double q = (double)S / (double)n;
    const unsigned long long frame = frame0 + (unsigned long long)f;
    int best_cnt = -1;
    double best_x[6] = {0, 0, 0, 0, 0, 0};
    // keep[k] -> sQ, in point order; returns the subset size (wave-uniform)
    auto compact = [&](auto keep) {
        int nq = 0;
        __syncthreads();
        for (int base = 0; base < n; base += 64) {
            const int k = base + lane;
            const bool take = k < n && keep(k);
            const unsigned long long b = __ballot(take);
            if (take) {
                const int pos = nq + __popcll(b & ((1ull << lane) - 1ull));
                sQ[3 * pos] = sP[3 * k]; sQ[3 * pos + 1] = sP[3 * k + 1]; sQ[3 * pos + 2] = sP[3 * k + 2];
            }
            nq += __popcll(b);
        }
        __syncthreads();
        return nq;
    };
    for (int h = 0; h < H; h++) {
        const int nq = compact([&](int k) {
            return h == 0 || ((double)(ransac_hash(seed, frame, (unsigned long long)h, (unsigned long long)k) >> 11) * 0x1.0p-53) < q;
        });
        if (nq < 6) continue;
        double xh[6], fh;
        int it, ev;
        const double fq0 = cyl_objective(x0, Pts{sQ, nq}, R, lane);
        fit_lm(sQ, nq, R, lane, tolx, tolf, hyp_iters, x0, fq0, xh, fh, it, ev);
        int c = 0;
        for (int k = lane; k < n; k += 64) c += ransac_inlier(sP, k, xh, R, tau) ? 1 : 0;
        c = wave_sum_i(c);
        if (c > best_cnt) {
            best_cnt = c;
#pragma unroll
            for (int k = 0; k < 6; k++) best_x[k] = xh[k];
        }
    }
    if (best_cnt < 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) best_x[k] = x0[k];
    }
    int nq = compact([&](int k) { return ransac_inlier(sP, k, best_x, R, tau); });
    const int n_inl = nq;
    const bool all_points = nq < 6;   // too few inliers to fit: all points, and say so in the mask
    if (all_points) nq = compact([&](int) { return true; });
    const double fs = cyl_objective(best_x, Pts{sQ, nq}, R, lane);
    double xf[6], ffinal;
    int itercount, func_evals;
    if constexpr (MODE == 0) fit_nm(sQ, nq, R, lane, tolx, tolf, maxiter, maxfun, best_x, fs, xf, ffinal, itercount, func_evals);
    else fit_lm(sQ, nq, R, lane, tolx, tolf, maxiter, best_x, fs, xf, ffinal, itercount, func_evals);
    if (!fit_finite(xf, ffinal)) { few_points(); return; }
    for (int k = lane; k < n; k += 64) mk[k] = all_points ? 1 : (ransac_inlier(sP, k, best_x, R, tau) ? 1 : 0);
    out.write_ok(f, lane, sQ, nq, x0, xf, f0, ffinal, itercount, func_evals);
    if (lane == 0) o_ninl[f] = n_inl;
}

}  // namespace

namespace {
// triangulate(matchedPoints1, matchedPoints2, stereoParams) for n frames of already matched pairs (fitSingleCylinder.m:15-17):
// one wavefront per frame, one lane per point; meanError through the same 64-lane tree as everywhere else
__global__ __launch_bounds__(64) void k_triangulate(const double *__restrict__ p1, const double *__restrict__ p2,
                                                    const int *__restrict__ cnt, const double *__restrict__ K1,
                                                    const double *__restrict__ K2, const double *__restrict__ T21,
                                                    double *__restrict__ o_X, double *__restrict__ o_err, double *__restrict__ o_mean_err)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int m = min(max(cnt[f], 0), MAXP);
    double P1[12], P2[12];
    {
        const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        double k1[9], k2[9], tt[16];
        for (int k = 0; k < 9; k++) { k1[k] = K1[k]; k2[k] = K2[k]; }
        for (int k = 0; k < 16; k++) tt[k] = T21[k];
        make_P(k1, I4, P1);
        make_P(k2, tt, P2);
    }
    double es = 0.0;
    for (int k = lane; k < m; k += 64) {
        const size_t o = (size_t)f * MAXP + k;
        double X[3], e;
        triangulate_one(P1, P2, p1[2 * o], p1[2 * o + 1], p2[2 * o], p2[2 * o + 1], X, e);
        o_X[3 * o] = X[0]; o_X[3 * o + 1] = X[1]; o_X[3 * o + 2] = X[2];
        o_err[o] = e;
        es = es + e;
    }
    es = wave_sum(es);
    if (lane == 0) o_mean_err[f] = m > 0 ? es / (double)m : 0.0;
}
}  // namespace

extern "C" size_t cpe_fit_workspace_bytes(int32_t n)
{
    // index tables of the selector + room for the by-products cpe_choose_idx_batch does not hand out (X, err, mean_err)
    return (size_t)(n > 0 ? n : 0) * (2 * TBL * TBL * sizeof(int) + (size_t)MAXP * 4 * sizeof(double) + sizeof(double));
}

extern "C" int32_t cpe_select_triangulate_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1,
                                                const double *xy2, const int32_t *id2, const int32_t *cnt2,
                                                int32_t n, const double *K1, const double *K2, const double *T21,
                                                int32_t selector, int32_t patch, double th, void *ws, size_t ws_bytes,
                                                double *p1, double *p2, int32_t *idx, double *X, double *err,
                                                int32_t *m, double *mean_err, int32_t *flags, void *stream)
{
    CPE_CHECK_ARG(xy1 && id1 && cnt1 && xy2 && id2 && cnt2 && K1 && K2 && T21 && p1 && p2 && idx && X && err && m &&
                      mean_err && flags,
                  "cpe_select_triangulate_batch: null pointer");
    CPE_CHECK_ARG(n >= 0, "cpe_select_triangulate_batch: n < 0");
    CPE_CHECK_ARG(selector >= 0 && selector <= 2, "cpe_select_triangulate_batch: selector must be 0,1,2");
    CPE_CHECK_ARG(patch >= 1 && patch <= 8, "cpe_select_triangulate_batch: patch must be 1..8");
    if (n == 0) return CPE_OK;
    if (!ws || ws_bytes < cpe_fit_workspace_bytes(n)) {
        cpe::set_error("cpe_select_triangulate_batch: workspace too small (%zu < %zu)", ws_bytes, cpe_fit_workspace_bytes(n));
        return CPE_ERR_WORKSPACE;
    }
    CPE_LAUNCH_BEGIN();
    CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_select_triangulate), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEL_LDS_BYTES));
    CPE_KLAUNCH(k_select_triangulate, dim3(n), dim3(64), SEL_LDS_BYTES, (hipStream_t)stream, xy1, id1, cnt1, xy2, id2, cnt2,
                       K1, K2, T21, selector, patch, th, (int *)ws, p1, p2, idx, X, err, m, mean_err, flags);
    CPE_CHECK_LAUNCH("k_select_triangulate");
    return CPE_OK;
}

extern "C" int32_t cpe_choose_idx_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                        const int32_t *id2, const int32_t *cnt2, int32_t n, const double *K1, const double *K2,
                                        const double *T21, int32_t patch, double th, void *ws, size_t ws_bytes, double *p1,
                                        double *p2, int32_t *idx, int32_t *m, int32_t *flags, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_choose_idx_batch: n < 0");
    if (n == 0) return CPE_OK;
    // refused here, under this entry's name, and not by the call below under the other one
    CPE_CHECK_ARG(patch >= 1 && patch <= 8, "cpe_choose_idx_batch: patch must be 1..8");
    if (!ws || ws_bytes < cpe_fit_workspace_bytes(n)) {
        cpe::set_error("cpe_choose_idx_batch: workspace too small (%zu < %zu)", ws_bytes, cpe_fit_workspace_bytes(n));
        return CPE_ERR_WORKSPACE;
    }
    // the selector triangulates every candidate anyway: its points and errors land in the workspace behind the index tables
    double *X = reinterpret_cast<double *>(static_cast<char *>(ws) + (size_t)n * 2 * TBL * TBL * sizeof(int));
    double *err = X + (size_t)n * MAXP * 3, *mean_err = err + (size_t)n * MAXP;
    return cpe_select_triangulate_batch(xy1, id1, cnt1, xy2, id2, cnt2, n, K1, K2, T21, CPE_SEL_CHOOSE_IDX, patch, th, ws, ws_bytes,
                                        p1, p2, idx, X, err, m, mean_err, flags, stream);
}

extern "C" int32_t cpe_triangulate_batch(const double *p1, const double *p2, const int32_t *cnt, int32_t n, const double *K1,
                                         const double *K2, const double *T21, double *X, double *err, double *mean_err,
                                         void *stream)
{
    CPE_CHECK_ARG(p1 && p2 && cnt && K1 && K2 && T21 && X && err && mean_err, "cpe_triangulate_batch: null pointer");
    CPE_CHECK_ARG(n >= 0, "cpe_triangulate_batch: n < 0");
    if (n == 0) return CPE_OK;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_triangulate, dim3(n), dim3(64), 0, (hipStream_t)stream, p1, p2, cnt, K1, K2, T21, X, err, mean_err);
    CPE_CHECK_LAUNCH("k_triangulate");
    return CPE_OK;
}

extern "C" int32_t cpe_fit_cylinder_batch(const double *X, const int32_t *cnt, int32_t n, double radius,
                                          const CpeFitParams *params, double *cyl_raw, double *cyl, double *T,
                                          double *fvals, int32_t *iters, int32_t *status, void *stream)
{
    CPE_CHECK_ARG(X && cnt && cyl_raw && cyl && T && fvals && iters && status, "cpe_fit_cylinder_batch: null pointer");
    CPE_CHECK_ARG(n >= 0, "cpe_fit_cylinder_batch: n < 0");
    CpeFitParams p = {1e-5, 1e-5, 100000, 100000, CPE_FIT_NELDER_MEAD, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.tol_x >= 0 && p.tol_f >= 0 && p.max_iter > 0 && p.max_fun_evals > 0,
                  "cpe_fit_cylinder_batch: bad CpeFitParams");
    if (n == 0) return CPE_OK;
    CPE_LAUNCH_BEGIN();
    CPE_CHECK_ARG(p.mode == CPE_FIT_NELDER_MEAD || p.mode == CPE_FIT_LM, "cpe_fit_cylinder_batch: unknown mode %d", p.mode);
    CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fit_cylinder<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FIT_LDS_BYTES));
    CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fit_cylinder<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FIT_LDS_BYTES));
    const FitOut out{cyl_raw, cyl, T, fvals, iters, status};
    if (p.mode == CPE_FIT_LM)
        CPE_KLAUNCH(k_fit_cylinder<1>, dim3(n), dim3(64), FIT_LDS_BYTES, (hipStream_t)stream, X, cnt, radius, p.tol_x, p.tol_f, p.max_iter,
                    p.max_fun_evals, out);
    else
        CPE_KLAUNCH(k_fit_cylinder<0>, dim3(n), dim3(64), FIT_LDS_BYTES, (hipStream_t)stream, X, cnt, radius, p.tol_x, p.tol_f, p.max_iter,
                    p.max_fun_evals, out);
    CPE_CHECK_LAUNCH("k_fit_cylinder");
    return CPE_OK;
}

extern "C" int32_t cpe_fit_cylinder_ransac_batch(const double *X, const int32_t *cnt, int32_t n, double radius,
                                                 const CpeFitParams *params, const CpeRansacParams *ransac, double *cyl_raw,
                                                 double *cyl, double *T, double *fvals, int32_t *iters, int32_t *status,
                                                 int32_t *n_inliers, uint8_t *inlier_mask, void *stream)
{
    CPE_CHECK_ARG(X && cnt && cyl_raw && cyl && T && fvals && iters && status && n_inliers && inlier_mask,
                  "cpe_fit_cylinder_ransac_batch: null pointer");
    CPE_CHECK_ARG(n >= 0, "cpe_fit_cylinder_ransac_batch: n < 0");
    CpeFitParams p = {1e-5, 1e-5, 100000, 100000, CPE_FIT_LM, 0};
    if (params) p = *params;
    CpeRansacParams r = {64, 12, 0.5, 0, 0, 8, 0};
    if (ransac) r = *ransac;
    CPE_CHECK_ARG(p.tol_x >= 0 && p.tol_f >= 0 && p.max_iter > 0 && p.max_fun_evals > 0, "cpe_fit_cylinder_ransac_batch: bad CpeFitParams");
    CPE_CHECK_ARG(p.mode == CPE_FIT_NELDER_MEAD || p.mode == CPE_FIT_LM, "cpe_fit_cylinder_ransac_batch: unknown mode %d", p.mode);
    CPE_CHECK_ARG(r.hypotheses >= 1 && r.hypotheses <= 4096 && r.sample >= 6 && r.tau > 0 && r.hyp_iters >= 1,
                  "cpe_fit_cylinder_ransac_batch: bad CpeRansacParams (hypotheses 1..4096, sample >= 6, tau > 0, hyp_iters >= 1)");
    if (n == 0) return CPE_OK;
    CPE_LAUNCH_BEGIN();
    CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fit_ransac<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RANSAC_LDS_BYTES));
    CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fit_ransac<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RANSAC_LDS_BYTES));
    const FitOut out{cyl_raw, cyl, T, fvals, iters, status};
    if (p.mode == CPE_FIT_LM)
        CPE_KLAUNCH(k_fit_ransac<1>, dim3(n), dim3(64), RANSAC_LDS_BYTES, (hipStream_t)stream, X, cnt, radius, r.hypotheses, r.sample, r.tau,
                    (unsigned long long)r.seed, (unsigned long long)r.frame0, r.hyp_iters, p.tol_x, p.tol_f, p.max_iter, p.max_fun_evals,
                    out, n_inliers, inlier_mask);
    else
        CPE_KLAUNCH(k_fit_ransac<0>, dim3(n), dim3(64), RANSAC_LDS_BYTES, (hipStream_t)stream, X, cnt, radius, r.hypotheses, r.sample, r.tau,
                    (unsigned long long)r.seed, (unsigned long long)r.frame0, r.hyp_iters, p.tol_x, p.tol_f, p.max_iter, p.max_fun_evals,
                    out, n_inliers, inlier_mask);
    CPE_CHECK_LAUNCH("k_fit_ransac");
    return CPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Row f-1: the multi-frame AGV-pose fit, utils/fitCylinderWPts3sAngs.m.  Its objective (:82-94, `dist`):
//   v = sum_i mean((d_i - R)^2),  d_i = getDistPts3ToLine(Pts3s{i}, line of T * TAGVcyls{i})
// k_multi_frame_terms : one wavefront per frame computes its term (same 64-lane reduction tree as the per-frame fit) for a
//                       Nelder-Mead driven from the host (cpe_amd/multiframe.py), which adds the F terms in frame order.
// k_multi_frame_fit   : the whole of fitCylinderWPts3sAngs for one group of frames per workgroup -- initial pose (:40-69),
//                       fminsearch (fit_nm_on, the body of the per-frame fit) on the same terms, vec2T of the result.
// k_multi_frame_lm    : build-defined fast mode of the same fit -- an initial pose from all kept frames in closed form, then
//                       Levenberg-Marquardt on the same objective (a handful of passes over the points).
// k_pose_vec2T/T2vec  : vec2T.m / T2vec.m for a batch of poses, the device functions the fit itself uses.
namespace {
// T_C1_cyl = T * TAGVcyls{i}: only column 2 (dy: the axis) and column 4 (org: the origin) are used
__device__ __forceinline__ void frame_axis(const double *T, const double *__restrict__ A, double *org, double *dy)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        dy[r] = ((T[r * 4] * A[1] + T[r * 4 + 1] * A[5]) + T[r * 4 + 2] * A[9]) + T[r * 4 + 3] * A[13];
        org[r] = ((T[r * 4] * A[3] + T[r * 4 + 1] * A[7]) + T[r * 4 + 2] * A[11]) + T[r * 4 + 3] * A[15];
    }
}

// one frame's term: mean((d - R)^2) over its points; T row-major vec2T(agvPose), A row-major getTAGVcyl of the frame.
// cnt is clamped to [0, MAXP]; a frame without points has the term 0.
__device__ __forceinline__ double multi_frame_term(const double *__restrict__ P, int cnt, const double *__restrict__ A, const double *T,
                                                   double R, int lane)
{
    const int n = min(max(cnt, 0), MAXP);
    if (n == 0) return 0.0;
    double org[3], dy[3], v[3], nv2;
    frame_axis(T, A, org, dy);
    axis_of(org, dy, v, nv2);
    double acc = 0.0;
    for (int k = lane; k < n; k += 64) {
        double d = dist_pt_line(P + 3 * k, org, v, nv2);
        double w = d - R;
        acc = acc + w * w;
    }
    acc = wave_sum(acc);
    return acc / (double)n;
}

__global__ __launch_bounds__(64) void k_multi_frame_terms(const double *__restrict__ X, const int *__restrict__ cnt,
                                                          const double *__restrict__ TAGV, const double *__restrict__ T,
                                                          double R, double *__restrict__ terms)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const double term = multi_frame_term(X + (size_t)f * MAXP * 3, cnt[f], TAGV + 16 * (size_t)f, T, R, lane);
    if (lane == 0) terms[f] = term;
}

// vec2T.m: rotvec2mat3d (premultiply form) of x[0..2] beside the translation x[3..5], row-major 4x4.  sin / cos are the
// device library's; everything else in the order of oracle/src/orc_fit.c::rotvec2mat.
__device__ __forceinline__ void pose_vec2T(const double *x, double *T)
{
    const double th = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    if (th < 1e-6) {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) T[r * 4 + q] = (r == q) ? 1.0 : 0.0;
    } else {
        const double u[3] = {x[0] / th, x[1] / th, x[2] / th};
        const double c = cos(th), s = sin(th), t = 1 - c;
        const double K[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) T[r * 4 + q] = (c * (r == q ? 1.0 : 0.0) + t * (u[r] * u[q])) + s * K[r * 3 + q];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) T[r * 4 + 3] = x[3 + r];
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}

// the near-pi branch of rotmat2vec3d with `a` the largest diagonal entry (constant indices: the arrays stay in registers)
template <int a>
__device__ __forceinline__ void rotvec_near_pi(const double *T, double th, double *v)
{
    constexpr int b = (a + 1) % 3, c = (a + 2) % 3;
    const double s = sqrt(T[a * 5] - T[b * 5] - T[c * 5] + 1);
    double w[3];
    w[a] = s / 2;
    w[b] = (T[b * 4 + a] + T[a * 4 + b]) / (2 * s);
    w[c] = (T[c * 4 + a] + T[a * 4 + c]) / (2 * s);
    const double nw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = th * w[k] / nw;
}

// T2vec.m: rotmat2vec3d (without its SVD re-orthogonalisation) of the rotation of a row-major 4x4, then the translation.
// Three branches as oracle/src/orc_fit.c::mat2rotvec: sin(theta) >= 1e-4, theta near 0, theta near pi.  acos / sin are the
// device library's.
__device__ __forceinline__ void pose_T2vec(const double *T, double *x)
{
    const double t = (T[0] + T[5]) + T[10];
    double ca = (t - 1) / 2;
    if (ca > 1) ca = 1;
    if (ca < -1) ca = -1;
    const double th = acos(ca);
    const double r[3] = {T[9] - T[6], T[2] - T[8], T[4] - T[1]};
    const double sth = sin(th);
    if (sth >= 1e-4) {
        const double vth = 1 / (2 * sth);
#pragma unroll
        for (int k = 0; k < 3; k++) x[k] = th * (r[k] * vth);
    } else if (t - 1 > 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) x[k] = (.5 - (t - 3) / 12) * r[k];
    } else {
        int a = 0;
        double daa = T[0];
        if (T[5] > daa) { a = 1; daa = T[5]; }
        if (T[10] > daa) a = 2;
        if (a == 0) rotvec_near_pi<0>(T, th, x);
        else if (a == 1) rotvec_near_pi<1>(T, th, x);
        else rotvec_near_pi<2>(T, th, x);
    }
#pragma unroll
    for (int r_ = 0; r_ < 3; r_++) x[3 + r_] = T[r_ * 4 + 3];
}

__device__ __forceinline__ void cross3(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// cylParams{i} of fitCylinderWPts3sAngs.m:40-47: the 2x6 [cylParams0; cylParams] indexed linearly (the reproduced quirk of
// applyCylParamsPrior.m:6-7), then applyCylParamsPrior with ymin over the frame's n >= 1 points (a wave min)
__device__ __forceinline__ void multi_prior(const double *__restrict__ M, const double *__restrict__ P, int n, int lane, double *cp)
{
    double ymin = DBL_MAX;
    for (int k = lane; k < n; k += 64) ymin = fmin(ymin, P[3 * k + 1]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ymin = fmin(ymin, __shfl_xor(ymin, off, 64));
    const double o[3] = {M[0], M[6], M[1]};
    double d[3] = {M[7], M[2], M[8]};
    if (d[1] < 0) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; }
    double t = 0;
    if (!(fabs(d[1]) < DBL_EPSILON)) t = (ymin - o[1]) / d[1];
#pragma unroll
    for (int c = 0; c < 3; c++) { cp[c] = o[c] + t * d[c]; cp[3 + c] = d[c]; }
}

// T0 of fitCylinderWPts3sAngs.m:48-69 as a pose vector: R = [dir1 en c1] / [y1 nd c2] by Gaussian elimination with row
// pivoting on B' R' = A' (the order of oracle/src/orc_fit.c::orc_multi_init and multiframe.initial_pose), t = origin1 - R p1.
// cp0 / cp1: multi_prior of the first two frames, A1 / A2 their getTAGVcyl.
__device__ __forceinline__ void multi_init(const double *cp0, const double *cp1, const double *__restrict__ A1,
                                           const double *__restrict__ A2, double *x0)
{
    const double p1[3] = {A1[3], A1[7], A1[11]}, p2[3] = {A2[3], A2[7], A2[11]};
    const double y1[3] = {A1[1], A1[5], A1[9]};
    const double d12[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    double nd[3], en[3], c1[3], c2[3];
    cross3(y1, d12, nd);
    const double nn = sqrt((nd[0] * nd[0] + nd[1] * nd[1]) + nd[2] * nd[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) nd[k] = nd[k] / nn;
    const double ed12[3] = {cp1[0] - cp0[0], cp1[1] - cp0[1], cp1[2] - cp0[2]};
    const double dir1[3] = {cp0[3], cp0[4], cp0[5]};
    cross3(dir1, ed12, en);
    const double ne = sqrt((en[0] * en[0] + en[1] * en[1]) + en[2] * en[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) en[k] = en[k] / ne;
    cross3(dir1, en, c1);
    cross3(y1, nd, c2);
    double Bt[9] = {y1[0], y1[1], y1[2], nd[0], nd[1], nd[2], c2[0], c2[1], c2[2]};
    double At[9] = {dir1[0], dir1[1], dir1[2], en[0], en[1], en[2], c1[0], c1[1], c1[2]};
    double Rt[9];
    gauss_solve<3, 3>(Bt, At, Rt);
    double T0[16];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T0[r * 4 + c] = Rt[c * 3 + r];
        const double s = (T0[r * 4] * p1[0] + T0[r * 4 + 1] * p1[1]) + T0[r * 4 + 2] * p1[2];
        T0[r * 4 + 3] = cp0[r] - s;
    }
    T0[12] = 0; T0[13] = 0; T0[14] = 0; T0[15] = 1;
    pose_T2vec(T0, x0);
}

constexpr int MF_WAVES = 4;               // wavefronts of a k_multi_frame_fit workgroup (512 VGPRs each: the simplex stays in registers)
constexpr int MF_MAXF = CPE_MULTI_MAXF;   // kept frames of one group

// dist() of fitCylinderWPts3sAngs.m:82-94 for a workgroup of MF_WAVES wavefronts that all evaluate the same pose: wave w
// computes the terms of kept frames w, w + MF_WAVES, ... (multi_frame_term: the bits of k_multi_frame_terms) into LDS, one
// barrier, then every wave adds the nk terms in kept-frame order.  The terms alternate between two LDS rows, so one barrier
// per evaluation is enough: a wave writes row p again only after the barrier of the evaluation in between, which no wave
// passes before all of them have read row p.  EVERY wave of the workgroup must make the same sequence of calls.
// WAVES: wavefronts of the workgroup (k_multi_frame_fit: MF_WAVES, k_multi_frame_lm: MFLM_WAVES).
template <int WAVES>
struct MultiObjectiveT {
    const double *X;
    const int *cnt;
    const double *TAGV;
    double R;
    const int *sIdx;   // LDS, kept frames in order
    double *sTerms;    // LDS, [2][MF_MAXF]
    int nk, wave, lane, row;
    __device__ double operator()(const double *x)
    {
        double T[16];
        pose_vec2T(x, T);
        double *t = sTerms + row * MF_MAXF;
        row ^= 1;
        for (int k = wave; k < nk; k += WAVES) {
            const int f = sIdx[k];
            const double term = multi_frame_term(X + (size_t)f * MAXP * 3, cnt[f], TAGV + 16 * (size_t)f, T, R, lane);
            if (lane == 0) t[k] = term;
        }
        __syncthreads();
        double v = 0.0;
        for (int k = 0; k < nk; k++) v = v + t[k];   // v = v + (vi*vi')/length(vi), :92
        return v;
    }
};
using MultiObjective = MultiObjectiveT<MF_WAVES>;

// the kept frames of [a, b) into sIdx, in order (one wavefront): counted past CAP, stored up to it.  -> the count
template <int CAP = MF_MAXF>
__device__ __forceinline__ int multi_kept_frames(const int *__restrict__ frame_ok, int a, int b, bool range_ok, int lane, int *sIdx)
{
    int nk = 0;
    if (range_ok)
        for (long long base = a; base < b; base += 64) {
            const long long f = base + lane;
            const bool keep = f < b && (frame_ok == nullptr || frame_ok[f] != 0);
            const unsigned long long bal = __ballot(keep);
            const int pos = nk + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && pos < CAP) sIdx[pos] = (int)f;
            nk += __popcll(bal);
        }
    return nk;
}

// the outputs of both multi-frame kernels, per group g; written by thread 0 of the workgroup
struct MultiOut {
    double *x0, *x, *T, *fvals;
    int *iters, *nused, *status;
    // a group that is not fitted: its status, every other output zero
    __device__ void write_failed(int g, int st) const
    {
        if (threadIdx.x != 0) return;
        for (int k = 0; k < 6; k++) { x0[6 * g + k] = 0; x[6 * g + k] = 0; }
        for (int k = 0; k < 16; k++) T[16 * g + k] = 0;
        fvals[2 * g] = 0; fvals[2 * g + 1] = 0;
        iters[2 * g] = 0; iters[2 * g + 1] = 0;
        nused[g] = 0;
        status[g] = st;
    }
    __device__ void write_ok(int g, const double *xs, const double *xf, double f0, double ffinal, int itercount, int func_evals, int nk) const
    {
        if (threadIdx.x != 0) return;
        double Tf[16];
        pose_vec2T(xf, Tf);
        for (int k = 0; k < 6; k++) { x0[6 * g + k] = xs[k]; x[6 * g + k] = xf[k]; }
        for (int k = 0; k < 16; k++) T[16 * g + k] = Tf[k];
        fvals[2 * g] = f0; fvals[2 * g + 1] = ffinal;
        iters[2 * g] = itercount; iters[2 * g + 1] = func_evals;
        nused[g] = nk;
        status[g] = CPE_ST_OK;
    }
};

// The head of the multi-frame kernels for group g: the kept frames of [group_start[g], group_start[g + 1]) into sIdx (LDS; sNk
// one int of LDS), one barrier.  -> their count nk >= 2, or 0 after the group's record is written: OVERFLOW for a range outside
// [0, n] or more than CAP kept frames (sIdx holds CAP), FEW_POINTS below two (assert(nAngles >= 2), fitCylinderWPts3sAngs.m:29)
// Out: MultiOut, or ConsensusOut with its further outputs
template <int CAP = MF_MAXF, class Out>
__device__ __forceinline__ int multi_group_begin(const int *__restrict__ frame_ok, const int *__restrict__ group_start, int n, int g,
                                                 int *sIdx, int *sNk, const Out &out)
{
    const int a = group_start[g], b = group_start[g + 1];
    const bool range_ok = 0 <= a && a <= b && b <= n;
    if (threadIdx.x < 64) {
        const int nk = multi_kept_frames<CAP>(frame_ok, a, b, range_ok, threadIdx.x, sIdx);
        if (threadIdx.x == 0) *sNk = nk;
    }
    __syncthreads();
    const int nk = *sNk;
    if (!range_ok || nk > CAP) { out.write_failed(g, CPE_ST_OVERFLOW); return 0; }
    if (nk < 2) { out.write_failed(g, CPE_ST_FEW_POINTS); return 0; }
    return nk;
}

// fitCylinderWPts3sAngs for group g = blockIdx.x: frames [group_start[g], group_start[g+1]) with frame_ok != 0.
// Barriers: one after the frame list, one per objective evaluation.  Every wave runs the same code on the same numbers --
// the frame list and the terms come from LDS, everything else each wave computes for itself, and the arithmetic is
// deterministic -- so every branch below, the simplex's included, goes the same way in all MF_WAVES waves and they execute
// the same barriers.  No barrier stands under a condition that depends on the wave or the lane.
__global__ __launch_bounds__(64 * MF_WAVES) void k_multi_frame_fit(
    const double *__restrict__ X, const int *__restrict__ cnt, const double *__restrict__ TAGV, const double *__restrict__ cyl_raw,
    const int *__restrict__ frame_ok, const int *__restrict__ group_start, int n, double R, double tolx, double tolf, int maxiter,
    int maxfun, const double *__restrict__ x0_in, const MultiOut out)
{
    __builtin_amdgcn_s_setprio(3);   // a long chain of dependent f64 operations on one CU (see k_fit_cylinder)
    __shared__ int sIdx[MF_MAXF];
    __shared__ double sTerms[2 * MF_MAXF];
    __shared__ int sNk;
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nk = multi_group_begin(frame_ok, group_start, n, g, sIdx, &sNk, out);
    if (nk == 0) return;
    const int fa = sIdx[0], fb = sIdx[1];
    const int na = min(max(cnt[fa], 0), MAXP), nb = min(max(cnt[fb], 0), MAXP);
    if (na < 1 || nb < 1) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    double x0[6];
    if (x0_in != nullptr) {
#pragma unroll
        for (int k = 0; k < 6; k++) x0[k] = x0_in[6 * (size_t)g + k];
    } else {
        double cp0[6], cp1[6];
        multi_prior(cyl_raw + 12 * (size_t)fa, X + (size_t)fa * MAXP * 3, na, lane, cp0);
        multi_prior(cyl_raw + 12 * (size_t)fb, X + (size_t)fb * MAXP * 3, nb, lane, cp1);
        multi_init(cp0, cp1, TAGV + 16 * (size_t)fa, TAGV + 16 * (size_t)fb, x0);
    }
    MultiObjective obj{X, cnt, TAGV, R, sIdx, sTerms, nk, wave, lane, 0};
    const double f0 = obj(x0);
    if (!fit_finite(x0, f0)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    double xf[6], ffinal;
    int itercount, func_evals;
    fit_nm_on(obj, tolx, tolf, maxiter, maxfun, x0, f0, xf, ffinal, itercount, func_evals);
    if (!fit_finite(xf, ffinal)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    out.write_ok(g, x0, xf, f0, ffinal, itercount, func_evals, nk);
}

// ---- BUILD-DEFINED (nothing like it in the reference, as the LM and RANSAC modes of the per-frame fit): the multi-frame fit by
// Levenberg-Marquardt from an initial pose made of all kept frames.  Same objective (MultiObjectiveT: the bits of
// cpe_multi_frame_terms added in kept-frame order), same 6-vector x, a handful of passes over the points instead of thousands.
#ifndef CPE_MFLM_WAVES
#define CPE_MFLM_WAVES 8
#endif
constexpr int MFLM_WAVES = CPE_MFLM_WAVES;    // wavefronts of a k_multi_frame_lm workgroup (4 / 8 / 16 measured)
constexpr int MFLM_SUMS = 27;    // upper triangle of J'J (21) and J'r (6)

// exp([w]x) = I + A [w]x + B [w]x^2 (row-major 3x3), A = sin(th)/th and B = (1 - cos th)/th^2 by their series below th = 1e-4:
// unlike pose_vec2T there is no angle below which the rotation is dropped, an LM step may be that small
__device__ __forceinline__ void rot_exp(const double *w, double *E)
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(th2);
    double A, B;
    if (th < 1e-4) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
    else { A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const double k2 = (K[r * 3] * K[q] + K[r * 3 + 1] * K[3 + q]) + K[r * 3 + 2] * K[6 + q];
            E[r * 3 + q] = ((r == q ? 1.0 : 0.0) + A * K[r * 3 + q]) + B * k2;
        }
}

// rotation matrix (row-major 3x3) of the quaternion (q0, qx, qy, qz), normalised here
__device__ __forceinline__ void quat2rot(const double *qin, double *Rm)
{
    const double nq = sqrt(((qin[0] * qin[0] + qin[1] * qin[1]) + qin[2] * qin[2]) + qin[3] * qin[3]);
    const double q0 = qin[0] / nq, qx = qin[1] / nq, qy = qin[2] / nq, qz = qin[3] / nq;
    Rm[0] = ((q0 * q0 + qx * qx) - qy * qy) - qz * qz; Rm[1] = 2 * (qx * qy - q0 * qz); Rm[2] = 2 * (qx * qz + q0 * qy);
    Rm[3] = 2 * (qy * qx + q0 * qz); Rm[4] = ((q0 * q0 - qx * qx) + qy * qy) - qz * qz; Rm[5] = 2 * (qy * qz - q0 * qx);
    Rm[6] = 2 * (qz * qx - q0 * qy); Rm[7] = 2 * (qz * qy + q0 * qx); Rm[8] = ((q0 * q0 - qx * qx) - qy * qy) + qz * qz;
}

// a kept frame the initial pose can use: at least one point, the fitted row of cyl_raw finite, its direction not zero.
// -> the origin o and the unit direction d of the fitted axis
__device__ __forceinline__ bool multi_usable(const int *__restrict__ cnt, const double *__restrict__ cyl_raw, int f, double *o, double *d)
{
    const double *row = cyl_raw + 12 * (size_t)f + 6;
    bool ok = cnt[f] >= 1;
#pragma unroll
    for (int k = 0; k < 3; k++) { o[k] = row[k]; d[k] = row[3 + k]; ok = ok && isfinite(o[k]) && isfinite(d[k]); }
    const double nd = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    ok = ok && isfinite(nd) && nd > 0;
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = d[k] / nd;
    return ok;
}

// The initial pose of the LM form, from all usable kept frames (in place of fitCylinderWPts3sAngs.m:40-69, which uses the first
// two and the linear-indexing quirk).  With o_i, d_i the fitted axis of frame i (d_i turned to the side of the first usable
// frame's), a_i / p_i columns 2 / 4 of its getTAGVcyl:
//   Rot(sigma) = the proper rotation maximising sum (Rot a_i).(sigma d_i): Horn's quaternion, the eigenvector of the largest
//                eigenvalue of N(S), S = sum a_i d_i'; N(-S) = -N(S), so sigma = -1 takes the smallest eigenvalue's
//   t(sigma)   = argmin sum |(I - d_i d_i')(Rot p_i + t - o_i)|^2: (sum P_i) t = sum P_i o_i - sum P_i Rot p_i, P_i = I - d_i d_i'
// Two passes over the kept frames, S first, then sum P_i and both right-hand sides: lane l adds kept frames l, l+64, ... in
// order, then the 64-lane tree.  Every wave of the workgroup computes the same numbers.  -> the two poses as vectors, the
// usable count.  (A fitted origin may lie far along its axis -- the simplex does not hold it -- and P_i o_i then carries the
// rounding of |o_i|: 1e10 mm gives about 1e-6 mm.  It is an initial pose.)
// A singular (sum P_i) (ridge 1e-12 trace as lm_damped_solve's, then a zero determinant) leaves NaN in that pose.
__device__ void multi_init_all(const int *__restrict__ cnt, const double *__restrict__ TAGV, const double *__restrict__ cyl_raw,
                               const int *sIdx, int nk, int lane, double *xp, double *xm, int &n_usable)
{
    // the first usable kept frame and the count
    int first = -1, nus = 0;
    for (int base = 0; base < nk; base += 64) {
        const int k = base + lane;
        double o[3], d[3];
        const bool us = k < nk && multi_usable(cnt, cyl_raw, sIdx[k], o, d);
        const unsigned long long bal = __ballot(us);
        if (first < 0 && bal != 0) first = sIdx[base + __ffsll((long long)bal) - 1];
        nus += __popcll(bal);
    }
    n_usable = nus;
    if (nus < 2) return;
    double o1[3], d1[3];
    multi_usable(cnt, cyl_raw, first, o1, d1);
    double S[9];
#pragma unroll
    for (int k = 0; k < 9; k++) S[k] = 0.0;
    for (int k = lane; k < nk; k += 64) {
        const int f = sIdx[k];
        double o[3], d[3];
        if (!multi_usable(cnt, cyl_raw, f, o, d)) continue;
        if ((d[0] * d1[0] + d[1] * d1[1]) + d[2] * d1[2] < 0) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; }
        const double *A = TAGV + 16 * (size_t)f;
        const double a[3] = {A[1], A[5], A[9]};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) S[r * 3 + c] = S[r * 3 + c] + a[r] * d[c];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) S[k] = wave_sum(S[k]);
    // Horn's N(S), S[r*3+c] = sum a_r d_c
    const double N[16] = {(S[0] + S[4]) + S[8], S[5] - S[7], S[6] - S[2], S[1] - S[3],
                          S[5] - S[7], (S[0] - S[4]) - S[8], S[1] + S[3], S[6] + S[2],
                          S[6] - S[2], S[1] + S[3], (S[4] - S[0]) - S[8], S[5] + S[7],
                          S[1] - S[3], S[6] + S[2], S[5] + S[7], (S[8] - S[0]) - S[4]};
    double w[4], V[16];
    jacobi_eig<4>(N, w, V);
    double qp[4] = {V[0], V[4], V[8], V[12]}, qm[4] = {V[0], V[4], V[8], V[12]}, wp = w[0], wm = w[0];
#pragma unroll
    for (int j = 1; j < 4; j++) {
        if (w[j] > wp) { wp = w[j]; qp[0] = V[j]; qp[1] = V[4 + j]; qp[2] = V[8 + j]; qp[3] = V[12 + j]; }
        if (w[j] < wm) { wm = w[j]; qm[0] = V[j]; qm[1] = V[4 + j]; qm[2] = V[8 + j]; qm[3] = V[12 + j]; }
    }
    double Rp[9], Rn[9];
    quat2rot(qp, Rp);
    quat2rot(qm, Rn);
    // second pass: sum P_i (upper triangle 00 01 02 11 12 22) and sum P_i (o_i - Rot p_i) for both rotations
    double M[6], bp[3], bm[3];
#pragma unroll
    for (int k = 0; k < 6; k++) M[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) { bp[k] = 0.0; bm[k] = 0.0; }
    for (int k = lane; k < nk; k += 64) {
        const int f = sIdx[k];
        double o[3], d[3];
        if (!multi_usable(cnt, cyl_raw, f, o, d)) continue;   // (the sign of d does not matter to d d')
        const double *A = TAGV + 16 * (size_t)f;
        const double p[3] = {A[3], A[7], A[11]};
        const double Pm[6] = {1.0 - d[0] * d[0], -(d[0] * d[1]), -(d[0] * d[2]), 1.0 - d[1] * d[1], -(d[1] * d[2]), 1.0 - d[2] * d[2]};
#pragma unroll
        for (int q = 0; q < 6; q++) M[q] = M[q] + Pm[q];
#pragma unroll
        for (int sg = 0; sg < 2; sg++) {
            const double *Rm = sg == 0 ? Rp : Rn;
            double *bs = sg == 0 ? bp : bm;
            double u[3];
#pragma unroll
            for (int r = 0; r < 3; r++) u[r] = o[r] - ((Rm[r * 3] * p[0] + Rm[r * 3 + 1] * p[1]) + Rm[r * 3 + 2] * p[2]);
            bs[0] = bs[0] + ((Pm[0] * u[0] + Pm[1] * u[1]) + Pm[2] * u[2]);
            bs[1] = bs[1] + ((Pm[1] * u[0] + Pm[3] * u[1]) + Pm[4] * u[2]);
            bs[2] = bs[2] + ((Pm[2] * u[0] + Pm[4] * u[1]) + Pm[5] * u[2]);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) M[k] = wave_sum(M[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) { bp[k] = wave_sum(bp[k]); bm[k] = wave_sum(bm[k]); }
    // inverse of (sum P_i) + ridge by its adjugate (symmetric 3x3)
    const double ridge = 1e-12 * ((M[0] + M[3]) + M[5]);
    const double m00 = M[0] + ridge, m01 = M[1], m02 = M[2], m11 = M[3] + ridge, m12 = M[4], m22 = M[5] + ridge;
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    const double inv = (det == 0) ? NAN : 1.0 / det;
#pragma unroll
    for (int sg = 0; sg < 2; sg++) {
        const double *Rm = sg == 0 ? Rp : Rn, *rhs = sg == 0 ? bp : bm;
        double T0[16];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) T0[r * 4 + c] = Rm[r * 3 + c];
        T0[3] = ((c00 * rhs[0] + c01 * rhs[1]) + c02 * rhs[2]) * inv;
        T0[7] = ((c01 * rhs[0] + c11 * rhs[1]) + c12 * rhs[2]) * inv;
        T0[11] = ((c02 * rhs[0] + c12 * rhs[1]) + c22 * rhs[2]) * inv;
        T0[12] = 0; T0[13] = 0; T0[14] = 0; T0[15] = 1;
        pose_T2vec(T0, sg == 0 ? xp : xm);
    }
}

// The pose of the multi-frame fit as lm_minimize takes it: the objective is obj, a step is the left perturbation Rot <-
// exp([dw]x) Rot, t <- t + dt of the pose T = vec2T(x) that normal() was last called at.
// normal(): J'J (upper triangle, 21) and J'r (6) of the residuals r_ik = (d_ik - R) / sqrt(n_i).  With o = Rot p + t, v = Rot a,
// al, e, d of point_on_axis (the quantities of multi_frame_term):  dr/dt = -e/d,  dr/dw = -((Rot p + al v) x e)/d, both /
// sqrt(n_i) (CylProblem's dr/do and dr/dv through do = dw x Rot p + dt, dv = dw x v; the bottom row of getTAGVcyl is taken as
// 0 0 0 1).  Fixed order: wave w takes kept frames w, w + WAVES, ... in order, lane l of it their points l, l + 64, ..., all into
// one set of 27 registers; the 64-lane tree; one row of sJ[WAVES][27] per wave; one barrier; every wave adds the rows in wave
// order.  sJ is written again only after a later objective evaluation (an accepted step), whose barrier every wave passes
// after it has read the rows.  EVERY wave of the workgroup must make the same sequence of calls.
template <int WAVES>
struct MultiPoseProblem {
    MultiObjectiveT<WAVES> &obj;
    double *sJ;     // LDS, [WAVES][MFLM_SUMS]
    double T[16];
    __device__ __forceinline__ double operator()(const double *x) { return obj(x); }
    __device__ __forceinline__ void normal(const double *x, double *A, double *g)
    {
        pose_vec2T(x, T);
        double acc[MFLM_SUMS];
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) acc[k] = 0.0;
        for (int kf = obj.wave; kf < obj.nk; kf += WAVES) {
            const int f = obj.sIdx[kf];
            const int n = min(max(obj.cnt[f], 0), MAXP);
            if (n == 0) continue;
            const double *P = obj.X + (size_t)f * MAXP * 3, *Am = obj.TAGV + 16 * (size_t)f;
            double org[3], dy[3], q[3], v[3], nv2;
            frame_axis(T, Am, org, dy);
#pragma unroll
            for (int r = 0; r < 3; r++) q[r] = (T[r * 4] * Am[3] + T[r * 4 + 1] * Am[7]) + T[r * 4 + 2] * Am[11];
            axis_of(org, dy, v, nv2);
            const double sc = 1.0 / sqrt((double)n);
            for (int k = obj.lane; k < n; k += 64) {
                double al, e[3], dd;
                point_on_axis(P + 3 * k, org, v, nv2, al, e, dd);
                if (dd > 0) {
                    const double r = (dd - obj.R) * sc, c1 = -(sc / dd);
                    const double m[3] = {q[0] + v[0] * al, q[1] + v[1] * al, q[2] + v[2] * al};
                    double mxe[3];
                    cross3(m, e, mxe);
                    const double j[6] = {c1 * mxe[0], c1 * mxe[1], c1 * mxe[2], c1 * e[0], c1 * e[1], c1 * e[2]};
                    normal_accumulate<6>(j, r, acc);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) {
            const double s = wave_sum(acc[k]);
            if (obj.lane == 0) sJ[obj.wave * MFLM_SUMS + k] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) {
            double s = 0.0;
            for (int w = 0; w < WAVES; w++) s = s + sJ[w * MFLM_SUMS + k];
            if (k < 21) A[k] = s;
            else g[k - 21] = s;
        }
    }
    __device__ __forceinline__ bool candidate(const double *, const double *dl, double *xn) const
    {
        double E[9], Tn[16];
        rot_exp(dl, E);
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) Tn[r * 4 + c] = (E[r * 3] * T[c] + E[r * 3 + 1] * T[4 + c]) + E[r * 3 + 2] * T[8 + c];
            Tn[r * 4 + 3] = T[r * 4 + 3] + dl[3 + r];
        }
        Tn[12] = 0; Tn[13] = 0; Tn[14] = 0; Tn[15] = 1;
        pose_T2vec(Tn, xn);
        return true;
    }
};

// The LM form of fitCylinderWPts3sAngs for group g = blockIdx.x (frames as in k_multi_frame_fit).  Barriers: one after the
// frame list, one per objective evaluation, one per Jacobian pass; lm_minimize's comment says why all waves execute the same ones.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_multi_frame_lm(
    const double *__restrict__ X, const int *__restrict__ cnt, const double *__restrict__ TAGV, const double *__restrict__ cyl_raw,
    const int *__restrict__ frame_ok, const int *__restrict__ group_start, int n, double R, double tolx, double tolf, int maxiter,
    const double *__restrict__ x0_in, const MultiOut out, double *__restrict__ o_terms)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ int sIdx[MF_MAXF];
    __shared__ double sTerms[2 * MF_MAXF];
    __shared__ double sJ[WAVES * MFLM_SUMS];
    __shared__ int sNk;
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nk = multi_group_begin(frame_ok, group_start, n, g, sIdx, &sNk, out);
    if (nk == 0) return;
    MultiObjectiveT<WAVES> obj{X, cnt, TAGV, R, sIdx, sTerms, nk, wave, lane, 0};
    double x0[6], f0;
    int func_evals;
    if (x0_in != nullptr) {
#pragma unroll
        for (int k = 0; k < 6; k++) x0[k] = x0_in[6 * (size_t)g + k];
        f0 = obj(x0);
        func_evals = 1;
    } else {
        double xm[6];
        int n_usable;
        multi_init_all(cnt, TAGV, cyl_raw, sIdx, nk, lane, x0, xm, n_usable);
        if (n_usable < 2) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
        f0 = obj(x0);
        const double fm = obj(xm);
        func_evals = 2;
        if (!(f0 <= fm) && fm == fm) {   // the lower objective, a tie to sigma = +1
#pragma unroll
            for (int k = 0; k < 6; k++) x0[k] = xm[k];
            f0 = fm;
        }
    }
    if (!fit_finite(x0, f0)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    MultiPoseProblem<WAVES> prob{obj, sJ};
    double x[6], fx;
    int itercount;
    lm_minimize<6>(prob, x0, f0, tolx, tolf, maxiter, x, fx, itercount, func_evals);
    if (!fit_finite(x, fx)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    if (o_terms != nullptr) {   // the terms at the returned pose: one more evaluation (not counted), its row of sTerms
        const double *t = sTerms + obj.row * MF_MAXF;
        obj(x);
        for (int k = threadIdx.x; k < nk; k += 64 * WAVES) o_terms[sIdx[k]] = t[k];
    }
    out.write_ok(g, x0, x, f0, fx, itercount, func_evals, nk);
}

// ---- BUILD-DEFINED (include/cpe.h cpe_multi_frame_consensus_batch): the LM form above with a consensus over frames in front of
// it, for experiments that hold frames with status 0 and a wrong cylinder.  Every pair of usable frames (or max_hyp pairs spread
// over them) gives a pose in closed form -- multi_init_all on a list of two -- that is scored by the kept frames whose term at
// it lies below tau^2; the best pose's frames are fitted by the LM loop, its inliers are taken again, and so on.
// k_multi_frame_hyp       : one wavefront per (hypothesis, group): key (inlier count, sum of their terms) and pose -> workspace.
// k_multi_frame_consensus : one workgroup per group: arg-min over the keys, the refinement rounds, every output.
// Both are made of the pieces of k_multi_frame_lm: the one MultiObjectiveT of a workgroup is pointed at the list it is to add up
// (the pair, all kept frames, the inliers), so its two rows of sTerms keep alternating whatever the list.
constexpr int MFC_REC = 7;   // doubles of a hypothesis in the workspace: the sum of its inliers' terms, its pose

// R offsets per frame and H hypotheses for u >= 2 usable frames; dense: the offsets are 1..R = u/2, every unordered pair occurs
__device__ __forceinline__ void consensus_plan(int u, int max_hyp, int &R, int &H, bool &dense)
{
    R = max(1, max_hyp / u);
    dense = R >= u / 2;
    if (dense) R = u / 2;
    H = min(R * u, max_hyp);
}

// hypothesis h -> the places a != b of its two frames in the usable list.  The offsets stay within u/2: (a, a + off) and (a + off,
// a + off + (u - off)) are the same two frames, and a pose that differs from an earlier one by rounding alone would make the
// arg-min a matter of last bits.  false: the one case left, the offset u/2 of an even u names every pair twice and this is the
// second time -- the hypothesis is void
__device__ __forceinline__ bool consensus_pair(int h, int u, int R, bool dense, int &a, int &b)
{
    const int k = h / u;
    const int off = dense ? 1 + k : 1 + ((2 * k + 1) * (u / 2 - 1)) / (2 * R);
    a = h % u;
    b = (a + off) % u;
    return !(2 * off == u && a >= off);
}

// the usable (multi_usable) frames of the kept list into sU, in kept order (one wavefront).  -> their count
__device__ __forceinline__ int multi_usable_frames(const int *__restrict__ cnt, const double *__restrict__ cyl_raw, const int *sIdx, int nk,
                                                   int lane, int *sU)
{
    int nu = 0;
    for (int base = 0; base < nk; base += 64) {
        const int k = base + lane;
        double o[3], d[3];
        const bool us = k < nk && multi_usable(cnt, cyl_raw, sIdx[k], o, d);
        const unsigned long long bal = __ballot(us);
        if (us) sU[nu + __popcll(bal & ((1ull << lane) - 1ull))] = sIdx[k];
        nu += __popcll(bal);
    }
    return nu;
}

// The inliers of a pose among the kept frames, t[k] the term of kept frame k at it (a row of sTerms): cnt >= 1 and t[k] < tau2.
// Every thread runs the same loop on the same numbers.  -> their count; sum: their terms added in kept order; with list, thread 0
// stores their frame numbers there (the caller's barrier publishes them) and same tells whether they are prev[0..nprev)
__device__ __forceinline__ int multi_inliers(const double *t, const int *sIdx, const int *__restrict__ cnt, int nk, double tau2, double &sum,
                                             int *list, const int *prev, int nprev, bool &same)
{
    int c = 0;
    double s = 0.0;
    bool sm = true;
    for (int k = 0; k < nk; k++) {
        const int f = sIdx[k];
        const double tk = t[k];
        if (cnt[f] >= 1 && tk < tau2) {
            s = s + tk;
            if (list != nullptr) {
                if (prev != nullptr) sm = sm && c < nprev && prev[c] == f;
                if (threadIdx.x == 0) list[c] = f;
            }
            c++;
        }
    }
    sum = s;
    same = sm && c == nprev;
    return c;
}

// Hypothesis h = blockIdx.y of group g = blockIdx.x, one wavefront.  A group that k_multi_frame_consensus reports as failed, and a
// hypothesis past the group's H, write nothing; every h < H writes its record (count -1: void).  H <= (u / 2) u and u is at
// most the length of the group's range, so most of the wavefronts past H leave before they read a frame.
__global__ __launch_bounds__(64) void k_multi_frame_hyp(
    const double *__restrict__ X, const int *__restrict__ cnt, const double *__restrict__ TAGV, const double *__restrict__ cyl_raw,
    const int *__restrict__ frame_ok, const int *__restrict__ group_start, int n, double R, double tau2, int max_hyp,
    double *__restrict__ wrec, int *__restrict__ wcount)
{
    __shared__ int sIdx[MF_MAXF];
    __shared__ int sU[MF_MAXF];
    __shared__ double sTerms[2 * MF_MAXF];
    __shared__ int sPair[2];
    const int h = blockIdx.y, g = blockIdx.x, lane = threadIdx.x;
    const int ga = group_start[g], gb = group_start[g + 1];
    const bool range_ok = 0 <= ga && ga <= gb && gb <= n;
    if (!range_ok || (long long)h >= (long long)max((gb - ga) / 2, 1) * (gb - ga)) return;
    const int nk = multi_kept_frames(frame_ok, ga, gb, range_ok, lane, sIdx);
    if (!range_ok || nk > MF_MAXF || nk < 2) return;
    __syncthreads();
    const int u = multi_usable_frames(cnt, cyl_raw, sIdx, nk, lane, sU);
    if (u < 2) return;
    int Rr, H;
    bool dense;
    consensus_plan(u, max_hyp, Rr, H, dense);
    if (h >= H) return;
    __syncthreads();
    int a, b;
    const bool first = consensus_pair(h, u, Rr, dense, a, b);
    if (lane == 0) { sPair[0] = sU[a]; sPair[1] = sU[b]; }
    __syncthreads();
    double x[6], xm[6];
    int n_usable;
    multi_init_all(cnt, TAGV, cyl_raw, sPair, 2, lane, x, xm, n_usable);
    MultiObjectiveT<1> obj{X, cnt, TAGV, R, sPair, sTerms, 2, 0, lane, 0};
    double f0 = obj(x);
    const double fm = obj(xm);
    if (!(f0 <= fm) && fm == fm) {   // the lower objective over the pair, a tie to sigma = +1
#pragma unroll
        for (int k = 0; k < 6; k++) x[k] = xm[k];
        f0 = fm;
    }
    int count = -1;
    double sum = 0.0;
    if (first && fit_finite(x, f0)) {
        obj.sIdx = sIdx;
        obj.nk = nk;
        const double *t = sTerms + obj.row * MF_MAXF;
        obj(x);
        bool same;
        count = multi_inliers(t, sIdx, cnt, nk, tau2, sum, nullptr, nullptr, 0, same);
    }
    if (lane == 0) {
        const size_t slot = (size_t)g * max_hyp + h;
        wcount[slot] = count;
        wrec[slot * MFC_REC] = sum;
#pragma unroll
        for (int k = 0; k < 6; k++) wrec[slot * MFC_REC + 1 + k] = x[k];
    }
}

// the key (-count, sum, h) of hypothesis 1 lies before that of hypothesis 2
__device__ __forceinline__ bool consensus_before(int c1, double s1, int h1, int c2, double s2, int h2)
{
    if (c1 != c2) return c1 > c2;
    if (s1 != s2) return s1 < s2;
    return h1 < h2;
}

// the outputs of k_multi_frame_consensus per group g: MultiOut's and three more; written by thread 0 of the workgroup
struct ConsensusOut {
    MultiOut m;
    int *n_inliers, *info, *flags;
    __device__ void write_failed(int g, int st) const
    {
        m.write_failed(g, st);
        if (threadIdx.x != 0) return;
        n_inliers[g] = 0;
        for (int k = 0; k < 4; k++) info[4 * g + k] = 0;
        flags[g] = 0;
    }
    __device__ void write_ok(int g, const double *xs, const double *xf, double f0, double ffinal, int itercount, int func_evals, int nk,
                             int nfit, int h, int fa, int fb, int rounds, int fl) const
    {
        m.write_ok(g, xs, xf, f0, ffinal, itercount, func_evals, nk);
        if (threadIdx.x != 0) return;
        n_inliers[g] = nfit;
        info[4 * g] = h; info[4 * g + 1] = fa; info[4 * g + 2] = fb; info[4 * g + 3] = rounds;
        flags[g] = fl;
    }
};

// Group g = blockIdx.x.  Barriers: those of k_multi_frame_lm, one after the usable list, one after the arg-min, one after every
// inlier list.  As there, every wave runs the same code on the same numbers (lists, terms, sums and the waves' best keys come from
// LDS, the records from the workspace), so no barrier stands under a condition that depends on the wave or the lane.
// WAVES is k_multi_frame_lm's, so that a round has the bits of that kernel on the same list.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_multi_frame_consensus(
    const double *__restrict__ X, const int *__restrict__ cnt, const double *__restrict__ TAGV, const double *__restrict__ cyl_raw,
    const int *__restrict__ frame_ok, const int *__restrict__ group_start, int n, double R, double tolx, double tolf, int maxiter,
    double tau2, int max_hyp, int max_rounds, int min_inliers, const double *__restrict__ wrec, const int *__restrict__ wcount,
    const ConsensusOut out, int *__restrict__ o_inlier, double *__restrict__ o_terms)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ int sIdx[MF_MAXF];
    __shared__ int sU[MF_MAXF];
    __shared__ int sInl[2 * MF_MAXF];
    __shared__ double sTerms[2 * MF_MAXF];
    __shared__ double sJ[WAVES * MFLM_SUMS];
    __shared__ double sKs[WAVES];
    __shared__ int sKc[WAVES], sKh[WAVES];
    __shared__ int sNk, sNu;
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nk = multi_group_begin(frame_ok, group_start, n, g, sIdx, &sNk, out);
    if (nk == 0) return;
    if (wave == 0) {
        const int nu = multi_usable_frames(cnt, cyl_raw, sIdx, nk, lane, sU);
        if (lane == 0) sNu = nu;
    }
    __syncthreads();
    const int u = sNu;
    if (u < 2) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    int Rr, H;
    bool dense;
    consensus_plan(u, max_hyp, Rr, H, dense);

    // the smallest key: thread t takes h = t, t + 64 WAVES, ..., the 64-lane butterfly, the waves' bests through LDS.  The keys
    // are totally ordered (h is part of them), so the order of the comparisons does not matter
    const size_t slot0 = (size_t)g * max_hyp;
    int bc = -1, bh = INT_MAX;
    double bs = 0.0;
    for (int h = threadIdx.x; h < H; h += 64 * WAVES) {
        const int c = wcount[slot0 + h];
        const double s = wrec[(slot0 + h) * MFC_REC];
        if (c >= 0 && consensus_before(c, s, h, bc, bs, bh)) { bc = c; bs = s; bh = h; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int c = __shfl_xor(bc, off, 64), h = __shfl_xor(bh, off, 64);
        const double s = __shfl_xor(bs, off, 64);
        if (c >= 0 && consensus_before(c, s, h, bc, bs, bh)) { bc = c; bs = s; bh = h; }
    }
    if (lane == 0) { sKc[wave] = bc; sKs[wave] = bs; sKh[wave] = bh; }
    __syncthreads();
    bc = -1; bs = 0.0; bh = INT_MAX;
    for (int w = 0; w < WAVES; w++)
        if (sKc[w] >= 0 && consensus_before(sKc[w], sKs[w], sKh[w], bc, bs, bh)) { bc = sKc[w]; bs = sKs[w]; bh = sKh[w]; }
    if (bc < min_inliers) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }   // no valid hypothesis: bc = -1

    double x0[6], x[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { x0[k] = wrec[(slot0 + bh) * MFC_REC + 1 + k]; x[k] = x0[k]; }
    MultiObjectiveT<WAVES> obj{X, cnt, TAGV, R, sIdx, sTerms, nk, wave, lane, 0};
    MultiPoseProblem<WAVES> prob{obj, sJ};
    // S_0: the terms of every kept frame at x0 again (the bits the hypothesis kernel saw), as a list this time
    const double *tall = sTerms + obj.row * MF_MAXF;
    obj(x0);
    int cur = 0;
    double f0;
    bool same;
    int nS = multi_inliers(tall, sIdx, cnt, nk, tau2, f0, sInl, nullptr, 0, same);
    __syncthreads();
    if (nS < min_inliers) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    double fx = f0;
    int nfit = nS, fitcur = 0, rounds = 0, flags = 0, itercount = 0, func_evals = 0;
    for (int r = 1; r <= max_rounds; r++) {
        // k_multi_frame_lm with x0_in = x on the list S_(r-1)
        obj.sIdx = sInl + cur * MF_MAXF;
        obj.nk = nS;
        const double fs = obj(x);
        int it, fe = 1;
        if (!fit_finite(x, fs)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
        double xn[6], fn;
        lm_minimize<6>(prob, x, fs, tolx, tolf, maxiter, xn, fn, it, fe);
        if (!fit_finite(xn, fn)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
#pragma unroll
        for (int k = 0; k < 6; k++) x[k] = xn[k];
        fx = fn;
        nfit = nS; fitcur = cur; rounds = r;
        itercount += it; func_evals += fe;
        // S_r
        obj.sIdx = sIdx;
        obj.nk = nk;
        tall = sTerms + obj.row * MF_MAXF;
        obj(x);
        double sr;
        const int nnew = multi_inliers(tall, sIdx, cnt, nk, tau2, sr, sInl + (cur ^ 1) * MF_MAXF, sInl + cur * MF_MAXF, nS, same);
        __syncthreads();
        if (same) { flags |= CPE_CONSENSUS_CONVERGED; break; }
        if (nnew < min_inliers) { flags |= CPE_CONSENSUS_SHRUNK; break; }
        cur ^= 1;
        nS = nnew;
    }
    // per frame: the terms at x (tall: the last evaluation was over all kept frames at x), and whether the frame is in the list x
    // was fitted to -- a merge of two ascending lists
    if (o_terms != nullptr)
        for (int k = threadIdx.x; k < nk; k += 64 * WAVES) o_terms[sIdx[k]] = tall[k];
    if (threadIdx.x == 0) {
        const int *fl = sInl + fitcur * MF_MAXF;
        int p = 0;
        for (int k = 0; k < nk; k++) {
            const int f = sIdx[k];
            const bool in = p < nfit && fl[p] == f;
            if (in) p++;
            o_inlier[f] = in ? 1 : 0;
        }
    }
    int pa, pb;
    consensus_pair(bh, u, Rr, dense, pa, pb);
    out.write_ok(g, x0, x, f0, fx, itercount, func_evals, nk, nfit, bh, sU[pa], sU[pb], rounds, flags);
}

__global__ __launch_bounds__(64) void k_pose_vec2T(const double *__restrict__ x, int n, double *__restrict__ T)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double xi[6], Ti[16];
#pragma unroll
    for (int k = 0; k < 6; k++) xi[k] = x[6 * (size_t)i + k];
    pose_vec2T(xi, Ti);
#pragma unroll
    for (int k = 0; k < 16; k++) T[16 * (size_t)i + k] = Ti[k];
}

__global__ __launch_bounds__(64) void k_pose_T2vec(const double *__restrict__ T, int n, double *__restrict__ x)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double Ti[16], xi[6];
#pragma unroll
    for (int k = 0; k < 16; k++) Ti[k] = T[16 * (size_t)i + k];
    pose_T2vec(Ti, xi);
#pragma unroll
    for (int k = 0; k < 6; k++) x[6 * (size_t)i + k] = xi[k];
}

// ---------------------------------------------------------------------------------------------------------------
// BUILD-DEFINED (nothing like it in the reference): pan and tilt of a frame from a calibrated T_Cam_AGV, the inverse of
// exp_gridDetection.m:90-93, which forms T_Cam_AGV * getTAGVcyl(pan, tilt) from the nominal angles in the file names.
// agv_chain          : getTAGVcyl.m (default config) on the device, the full product of its five matrices.
// k_agv_chain        : that for a batch of angle pairs, one lane per pair.
// k_frame_angles_lm  : one wavefront per frame minimises the frame's term of the multi-frame objective over (pan, tilt) by
//                      Levenberg-Marquardt on two unknowns: lm_minimize's loop written out (see the kernel).

// getTAGVcyl.m: TAP * TPT0 * T01 * T12 * T2C in the operation order of cpe_amd/multiframe.py::get_TAGVcyl -- cos(pan), sin(pan),
// cos(-tilt), sin(-tilt), -tan(tilt) * L, every entry of a product as ((a*b + c*d) + e*f) + g*h.  sin / cos / tan are the
// device library's.  All indices are constants after unrolling: the matrices stay in registers.
__device__ __forceinline__ void agv_chain(double pan, double tilt, double *A)
{
    const double cp = cos(pan), sp = sin(pan), ct = cos(-tilt), st = sin(-tilt);
    const double L = sqrt((-143.1 * -143.1 + 0.0 * 0.0) + 0.0 * 0.0);
    const double mtr = -tan(tilt) * L;
    const double TPT0[16] = {1, 0, 0, -143.1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double T01[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, mtr, 0, 0, 0, 1};
    const double T12[16] = {ct, 0, st, 0, 0, 1, 0, 0, -st, 0, ct, 0, 0, 0, 0, 1};
    const double T2C[16] = {0, -1, 0, 321.1, -1, 0, 0, 0, 0, 0, -1, 110, 0, 0, 0, 1};
    double acc[16] = {cp, -sp, 0, 0, sp, cp, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, nxt[16];
#define CHAIN_TIMES(M)                                                                                                    \
    _Pragma("unroll") for (int r = 0; r < 4; r++) _Pragma("unroll") for (int c = 0; c < 4; c++)                           \
        nxt[r * 4 + c] = ((acc[r * 4] * M[c] + acc[r * 4 + 1] * M[4 + c]) + acc[r * 4 + 2] * M[8 + c]) + acc[r * 4 + 3] * M[12 + c]; \
    _Pragma("unroll") for (int k = 0; k < 16; k++) acc[k] = nxt[k];
    CHAIN_TIMES(TPT0)
    CHAIN_TIMES(T01)
    CHAIN_TIMES(T12)
    CHAIN_TIMES(T2C)
#undef CHAIN_TIMES
#pragma unroll
    for (int k = 0; k < 16; k++) A[k] = acc[k];
}

__global__ __launch_bounds__(64) void k_agv_chain(const double *__restrict__ angles, int n, double *__restrict__ TAGV)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double A[16];
    agv_chain(angles[2 * (size_t)i], angles[2 * (size_t)i + 1], A);
#pragma unroll
    for (int k = 0; k < 16; k++) TAGV[16 * (size_t)i + k] = A[k];
}

// d/dpan and d/dtilt of columns 2 (a) and 4 (p) of getTAGVcyl in closed form, for the Jacobian only (values always come from
// agv_chain).  With c = cos(-tilt), s = sin(-tilt) (dc/dtilt = s, ds/dtilt = -c):
//   a = Rz(pan) (-c, 0, s),  p = Rz(pan) (-143.1 + 321.1 c + 110 s, 0, -143.1 tan(tilt) - 321.1 s + 110 c)
// and d/dpan of Rz(pan) (x, 0, z) is (-sin(pan) x, cos(pan) x, 0).  -> da[0..2] / dp[0..2] by pan, da[3..5] / dp[3..5] by tilt
__device__ __forceinline__ void agv_chain_derivatives(double pan, double tilt, double *da, double *dp)
{
    const double cp = cos(pan), sp = sin(pan), c = cos(-tilt), s = sin(-tilt);
    const double ax = -c, px = (-143.1 + 321.1 * c) + 110.0 * s;
    const double dax = -s, daz = -c;
    const double dpx = 321.1 * s - 110.0 * c, dpz = (-143.1 / (c * c) + 321.1 * c) + 110.0 * s;
    da[0] = -sp * ax; da[1] = cp * ax; da[2] = 0.0;
    dp[0] = -sp * px; dp[1] = cp * px; dp[2] = 0.0;
    da[3] = cp * dax; da[4] = sp * dax; da[5] = daz;
    dp[3] = cp * dpx; dp[4] = sp * dpx; dp[5] = dpz;
}

// the outputs of the angle solver, per frame f (TAGV and Tcyl may be NULL)
struct AnglesOut {
    double *a0, *a, *fvals;
    int *iters;
    double *TAGV, *Tcyl;
    int *status;
    // a frame without angles: its status, every other output zero
    __device__ void write_failed(int f, int lane, int st) const
    {
        if (lane != 0) return;
        const size_t f2 = 2 * (size_t)f, f16 = 16 * (size_t)f;
        a0[f2] = 0; a0[f2 + 1] = 0; a[f2] = 0; a[f2 + 1] = 0;
        fvals[f2] = 0; fvals[f2 + 1] = 0; iters[f2] = 0; iters[f2 + 1] = 0;
        if (TAGV != nullptr)
            for (int k = 0; k < 16; k++) TAGV[f16 + k] = 0;
        if (Tcyl != nullptr)
            for (int k = 0; k < 16; k++) Tcyl[f16 + k] = 0;
        status[f] = st;
    }
};

// The frame's objective f(q) = multi_frame_term(P, cnt, agv_chain(q), T, R): the bits of cpe_agv_chain_batch +
// cpe_multi_frame_terms.  Frame f = blockIdx.x, one wavefront.  Every lane holds the same angles, sums and decisions (the
// sums come out of the 64-lane tree, everything else is computed from per-frame values), so every branch below goes the
// same way in all lanes and no wave-level operation stands under a lane-dependent condition.  Every loop is bounded whatever
// the data: min(maxiter, 200) iterations of at most 12 trials; a non-finite objective or candidate is a rejected trial.
// The loop is lm_minimize's, written out so that the objective, and with it the inlined agv_chain, has a single call site and
// the chain of an accepted candidate is kept for the Jacobian pass and the outputs.  Both forms under the driver were built
// and timed: keeping the accepted chain through a hook takes 1 wave/SIMD and 4 % / 24 % more time at 45 / 4096
// frames, recomputing the chain 16 % / 8 % more.
__global__ __launch_bounds__(64) void k_frame_angles_lm(
    const double *__restrict__ X, const int *__restrict__ cnt, const double *__restrict__ cyl_raw, const double *__restrict__ Tg,
    const int *__restrict__ pose_index, int G, double R, double tolx, double tolf, int maxiter, const double *__restrict__ a0_in,
    const AnglesOut out)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int pi = pose_index != nullptr ? pose_index[f] : 0;
    if (pi < 0 || pi >= G) { out.write_failed(f, lane, CPE_ST_OVERFLOW); return; }
    const int n = min(max(cnt[f], 0), MAXP);
    if (n < CPE_FIT_MIN_POINTS) { out.write_failed(f, lane, CPE_ST_FEW_POINTS); return; }
    const double *P = X + (size_t)f * MAXP * 3;
    double T[16];
#pragma unroll
    for (int k = 0; k < 16; k++) T[k] = Tg[16 * (size_t)pi + k];
    double q0[2];
    if (a0_in != nullptr) {
        q0[0] = a0_in[2 * (size_t)f];
        q0[1] = a0_in[2 * (size_t)f + 1];
    } else {
        // the chain's second column is Rz(pan) (-c, 0, s): a = Rot' d, turned to a_x <= 0 (|pan| < pi/2)
        double o[3], d[3];
        if (!multi_usable(cnt, cyl_raw, f, o, d)) { out.write_failed(f, lane, CPE_ST_FEW_POINTS); return; }
        double a[3];
#pragma unroll
        for (int k = 0; k < 3; k++) a[k] = (T[k] * d[0] + T[4 + k] * d[1]) + T[8 + k] * d[2];
        if (a[0] > 0) { a[0] = -a[0]; a[1] = -a[1]; a[2] = -a[2]; }
        q0[0] = atan2(-a[1], -a[0]);
        q0[1] = asin(fmin(fmax(-a[2], -1.0), 1.0));
    }
    // One call site for the objective (the chain's sin / cos / tan are the large part of this kernel): the candidate (c0, c1)
    // is first the start, then every trial of the LM.  lm_minimize's loop, flattened (its constants and rules, see there): a
    // new point (the start, an accepted trial) gets its Jacobian pass and opens an iteration of up to 12 trials.
    double A[16], q[2] = {q0[0], q0[1]}, c0 = q0[0], c1 = q0[1];
    double f0 = 0.0, fx = 0.0, fprev = 0.0, lambda = 1e-3, d[2] = {0.0, 0.0};
    double S[3] = {0.0, 0.0, 0.0}, g[2] = {0.0, 0.0};   // J'J (00 01 11) and J'r
    int itercount = 0, func_evals = 0, tr = 0;
    bool started = false;
    const double sc = 1.0 / sqrt((double)n);
    for (int step = 0; step < 1 + 12 * 200; step++) {
        double An[16];
        agv_chain(c0, c1, An);
        const double fn = multi_frame_term(P, n, An, T, R, lane);
        func_evals++;
        bool fresh = false;
        if (!started) {
            f0 = fn;
            fx = fn;
            started = true;
            if (!isfinite(fn)) break;
            fresh = true;
        } else if (fn < fx) {   // (false for a NaN objective)
            q[0] = c0; q[1] = c1;
            fx = fn;
            lambda = fmax(lambda / 10, 1e-12);
            if ((fprev - fx) <= tolf * 1e-3 * (1.0 + fx) && fmax(fabs(d[0]), fabs(d[1])) <= tolx) {
#pragma unroll
                for (int k = 0; k < 16; k++) A[k] = An[k];
                break;
            }
            fresh = true;
        } else {
            lambda = lambda * 10;
            tr++;
        }
        if (fresh) {
#pragma unroll
            for (int k = 0; k < 16; k++) A[k] = An[k];
            if (!(itercount < maxiter && itercount < 200)) break;
            // one pass: J'J (3 sums) and J'r (2), r_k = (d_k - R) / sqrt(n), dr/dq = dr/do . do/dq + dr/dv . dv/dq with CylProblem's
            // dr/do = -e/d, dr/dv = -(al/d) e and do/dq = Rot dp/dq, dv/dq = Rot da/dq
            double org[3], dy[3], da[6], dp[6], dob[6], dvb[6], v[3], nv2;
            agv_chain_derivatives(q[0], q[1], da, dp);
            frame_axis(T, A, org, dy);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    dob[3 * j + r] = (T[r * 4] * dp[3 * j] + T[r * 4 + 1] * dp[3 * j + 1]) + T[r * 4 + 2] * dp[3 * j + 2];
                    dvb[3 * j + r] = (T[r * 4] * da[3 * j] + T[r * 4 + 1] * da[3 * j + 1]) + T[r * 4 + 2] * da[3 * j + 2];
                }
            axis_of(org, dy, v, nv2);
            double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int k = lane; k < n; k += 64) {
                double al, e[3], dd;
                point_on_axis(P + 3 * k, org, v, nv2, al, e, dd);
                if (dd > 0) {
                    const double r = (dd - R) * sc, k1 = -(sc / dd), k2 = k1 * al;
                    const double j[2] = {k1 * ((e[0] * dob[0] + e[1] * dob[1]) + e[2] * dob[2]) + k2 * ((e[0] * dvb[0] + e[1] * dvb[1]) + e[2] * dvb[2]),
                                         k1 * ((e[0] * dob[3] + e[1] * dob[4]) + e[2] * dob[5]) + k2 * ((e[0] * dvb[3] + e[1] * dvb[4]) + e[2] * dvb[5])};
                    normal_accumulate<2>(j, r, acc);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) S[k] = wave_sum(acc[k]);
            g[0] = wave_sum(acc[3]);
            g[1] = wave_sum(acc[4]);
            itercount++;
            tr = 0;
            fprev = fx;
        }
        // the next trial.  A singular system or a candidate that is not finite or has |tilt| >= pi/2 - 1e-3 (tan(tilt) of the
        // chain has its pole at pi/2) is a rejected trial.
        bool have = false;
        for (; tr < 12 && !have;) {
            have = lm_damped_solve<2>(S, g, lambda, d);
            c0 = q[0] + d[0];
            c1 = q[1] + d[1];
            have = have && isfinite(c0) && isfinite(c1) && fabs(c1) < 1.5707963267948966 - 1e-3;
            if (!have) { lambda = lambda * 10; tr++; }
        }
        if (!have) break;
    }
    if (!(isfinite(q0[0]) && isfinite(q0[1]) && isfinite(f0) && isfinite(q[0]) && isfinite(q[1]) && isfinite(fx))) {
        out.write_failed(f, lane, CPE_ST_FEW_POINTS);
        return;
    }
    if (lane == 0) {
        const size_t f2 = 2 * (size_t)f, f16 = 16 * (size_t)f;
        out.a0[f2] = q0[0]; out.a0[f2 + 1] = q0[1]; out.a[f2] = q[0]; out.a[f2 + 1] = q[1];
        out.fvals[f2] = f0; out.fvals[f2 + 1] = fx;
        out.iters[f2] = itercount; out.iters[f2 + 1] = func_evals;
        if (out.TAGV != nullptr) {
#pragma unroll
            for (int k = 0; k < 16; k++) out.TAGV[f16 + k] = A[k];
        }
        if (out.Tcyl != nullptr) {   // T * chain, every entry in multi_frame_term's operation order
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++)
                    out.Tcyl[f16 + r * 4 + c] = ((T[r * 4] * A[c] + T[r * 4 + 1] * A[4 + c]) + T[r * 4 + 2] * A[8 + c]) + T[r * 4 + 3] * A[12 + c];
        }
        out.status[f] = CPE_ST_OK;
    }
}
}  // namespace

extern "C" int32_t cpe_multi_frame_terms(const double *X, const int32_t *cnt, int32_t n, const double *TAGVcyl,
                                         const double *T, double radius, double *terms, void *stream)
{
    CPE_CHECK_ARG(X && cnt && TAGVcyl && T && terms && n >= 0, "cpe_multi_frame_terms: bad argument");
    if (n == 0) return CPE_OK;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_multi_frame_terms, dim3(n), dim3(64), 0, (hipStream_t)stream, X, cnt, TAGVcyl, T, radius, terms);
    CPE_CHECK_LAUNCH("k_multi_frame_terms");
    return CPE_OK;
}

extern "C" int32_t cpe_multi_frame_fit_batch(const double *X, const int32_t *cnt, const double *TAGVcyl, const double *cyl_raw,
                                             const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n, double radius,
                                             const CpeFitParams *params, const double *x0_in, double *x0, double *x, double *T,
                                             double *fvals, int32_t *iters, int32_t *n_used, int32_t *status, void *stream)
{
    CPE_CHECK_ARG(X && cnt && TAGVcyl && group_start && x0 && x && T && fvals && iters && n_used && status,
                  "cpe_multi_frame_fit_batch: null pointer");
    CPE_CHECK_ARG(cyl_raw || x0_in, "cpe_multi_frame_fit_batch: cyl_raw may be NULL only beside x0_in");
    CPE_CHECK_ARG(G >= 0 && n >= 0, "cpe_multi_frame_fit_batch: G < 0 or n < 0");
    CpeFitParams p = {1e-5, 1e-5, 100000, 100000, CPE_FIT_NELDER_MEAD, 0};   // fitCylinderWPts3sAngs.m:75
    if (params) p = *params;
    CPE_CHECK_ARG(p.tol_x >= 0 && p.tol_f >= 0 && p.max_iter > 0 && p.max_fun_evals > 0, "cpe_multi_frame_fit_batch: bad CpeFitParams");
    CPE_CHECK_ARG(p.mode == CPE_FIT_NELDER_MEAD, "cpe_multi_frame_fit_batch: mode %d (the multi-frame fit is Nelder-Mead only)", p.mode);
    if (G == 0) return CPE_OK;
    CPE_LAUNCH_BEGIN();
    const MultiOut out{x0, x, T, fvals, iters, n_used, status};
    CPE_KLAUNCH(k_multi_frame_fit, dim3(G), dim3(64 * MF_WAVES), 0, (hipStream_t)stream, X, cnt, TAGVcyl, cyl_raw, frame_ok, group_start,
                n, radius, p.tol_x, p.tol_f, p.max_iter, p.max_fun_evals, x0_in, out);
    CPE_CHECK_LAUNCH("k_multi_frame_fit");
    return CPE_OK;
}

extern "C" int32_t cpe_multi_frame_fit_lm_batch(const double *X, const int32_t *cnt, const double *TAGVcyl, const double *cyl_raw,
                                                const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n, double radius,
                                                const CpeFitParams *params, const double *x0_in, double *x0, double *x, double *T,
                                                double *fvals, int32_t *iters, int32_t *n_used, int32_t *status, double *frame_terms,
                                                void *stream)
{
    CPE_CHECK_ARG(X && cnt && TAGVcyl && group_start && x0 && x && T && fvals && iters && n_used && status,
                  "cpe_multi_frame_fit_lm_batch: null pointer");
    CPE_CHECK_ARG(cyl_raw || x0_in, "cpe_multi_frame_fit_lm_batch: cyl_raw may be NULL only beside x0_in");
    CPE_CHECK_ARG(G >= 0 && n >= 0, "cpe_multi_frame_fit_lm_batch: G < 0 or n < 0");
    CpeFitParams p = {1e-5, 1e-5, 100000, 100000, CPE_FIT_LM, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.tol_x >= 0 && p.tol_f >= 0 && p.max_iter > 0, "cpe_multi_frame_fit_lm_batch: bad CpeFitParams");
    CPE_CHECK_ARG(p.mode == CPE_FIT_LM, "cpe_multi_frame_fit_lm_batch: mode %d (this is the LM form; Nelder-Mead is cpe_multi_frame_fit_batch)",
                  p.mode);
    if (G == 0) return CPE_OK;
    CPE_LAUNCH_BEGIN();
    const MultiOut out{x0, x, T, fvals, iters, n_used, status};
    CPE_KLAUNCH(k_multi_frame_lm<MFLM_WAVES>, dim3(G), dim3(64 * MFLM_WAVES), 0, (hipStream_t)stream, X, cnt, TAGVcyl, cyl_raw, frame_ok,
                group_start, n, radius, p.tol_x, p.tol_f, p.max_iter, x0_in, out, frame_terms);
    CPE_CHECK_LAUNCH("k_multi_frame_lm");
    return CPE_OK;
}

extern "C" size_t cpe_multi_frame_consensus_workspace_bytes(int32_t G, int32_t max_hyp)
{
    if (G <= 0 || max_hyp < 1 || max_hyp > CPE_CONSENSUS_MAX_HYP) return 0;
    return (size_t)G * max_hyp * (MFC_REC * sizeof(double) + sizeof(int));
}

extern "C" int32_t cpe_multi_frame_consensus_batch(const double *X, const int32_t *cnt, const double *TAGVcyl, const double *cyl_raw,
                                                   const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n, double radius,
                                                   const CpeFitParams *params, const CpeConsensusParams *cons, void *ws, size_t ws_bytes,
                                                   double *x0, double *x, double *T, double *fvals, int32_t *iters, int32_t *n_used,
                                                   int32_t *n_inliers, int32_t *info, int32_t *flags, int32_t *status, int32_t *inlier,
                                                   double *frame_terms, void *stream)
{
    CPE_CHECK_ARG(X && cnt && TAGVcyl && cyl_raw && group_start && x0 && x && T && fvals && iters && n_used && n_inliers && info && flags &&
                  status && inlier, "cpe_multi_frame_consensus_batch: null pointer");
    CPE_CHECK_ARG(G >= 0 && n >= 0, "cpe_multi_frame_consensus_batch: G < 0 or n < 0");
    CpeFitParams p = {1e-5, 1e-5, 100000, 100000, CPE_FIT_LM, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.tol_x >= 0 && p.tol_f >= 0 && p.max_iter > 0, "cpe_multi_frame_consensus_batch: bad CpeFitParams");
    CPE_CHECK_ARG(p.mode == CPE_FIT_LM, "cpe_multi_frame_consensus_batch: mode %d (the refinement is Levenberg-Marquardt only)", p.mode);
    CpeConsensusParams c = {0.5, 2048, 4, 3};
    if (cons) c = *cons;
    CPE_CHECK_ARG(c.tau > 0 && c.tau <= DBL_MAX && c.max_hyp >= 1 && c.max_hyp <= CPE_CONSENSUS_MAX_HYP && c.max_rounds >= 0 &&
                  c.max_rounds <= 16 && c.min_inliers >= 2,
                  "cpe_multi_frame_consensus_batch: bad CpeConsensusParams (tau > 0, max_hyp 1..%d, max_rounds 0..16, min_inliers >= 2)",
                  CPE_CONSENSUS_MAX_HYP);
    if (G == 0) return CPE_OK;
    const size_t need = cpe_multi_frame_consensus_workspace_bytes(G, c.max_hyp);
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < need) {
        cpe::set_error("cpe_multi_frame_consensus_batch: workspace missing, not 8-byte aligned or too small (%zu < %zu)", ws_bytes, need);
        return CPE_ERR_WORKSPACE;
    }
    CPE_LAUNCH_BEGIN();
    double *wrec = (double *)ws;
    int *wcount = (int *)(wrec + (size_t)G * c.max_hyp * MFC_REC);
    const double tau2 = c.tau * c.tau;
    // no group has more than min(n, MF_MAXF) usable frames, so none has a hypothesis at or past (u / 2) u of that
    const long long umax = n < MF_MAXF ? n : MF_MAXF, most = (umax / 2 > 1 ? umax / 2 : 1) * (umax > 1 ? umax : 1);
    const int hyp_rows = most < c.max_hyp ? (int)most : c.max_hyp;
    CPE_KLAUNCH(k_multi_frame_hyp, dim3(G, hyp_rows), dim3(64), 0, (hipStream_t)stream, X, cnt, TAGVcyl, cyl_raw, frame_ok, group_start, n,
                radius, tau2, c.max_hyp, wrec, wcount);
    CPE_CHECK_LAUNCH("k_multi_frame_hyp");
    const ConsensusOut out{MultiOut{x0, x, T, fvals, iters, n_used, status}, n_inliers, info, flags};
    CPE_KLAUNCH(k_multi_frame_consensus<MFLM_WAVES>, dim3(G), dim3(64 * MFLM_WAVES), 0, (hipStream_t)stream, X, cnt, TAGVcyl, cyl_raw,
                frame_ok, group_start, n, radius, p.tol_x, p.tol_f, p.max_iter, tau2, c.max_hyp, c.max_rounds, c.min_inliers, wrec, wcount, out,
                inlier, frame_terms);
    CPE_CHECK_LAUNCH("k_multi_frame_consensus");
    return CPE_OK;
}

extern "C" int32_t cpe_pose_vec2T_batch(const double *x, int32_t n, double *T, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_pose_vec2T_batch: n < 0");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(x && T, "cpe_pose_vec2T_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_pose_vec2T, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, n, T);
    CPE_CHECK_LAUNCH("k_pose_vec2T");
    return CPE_OK;
}

extern "C" int32_t cpe_pose_T2vec_batch(const double *T, int32_t n, double *x, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_pose_T2vec_batch: n < 0");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(T && x, "cpe_pose_T2vec_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_pose_T2vec, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, T, n, x);
    CPE_CHECK_LAUNCH("k_pose_T2vec");
    return CPE_OK;
}

extern "C" int32_t cpe_agv_chain_batch(const double *angles, int32_t n, double *TAGVcyl, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_agv_chain_batch: n < 0");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(angles && TAGVcyl, "cpe_agv_chain_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_agv_chain, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, angles, n, TAGVcyl);
    CPE_CHECK_LAUNCH("k_agv_chain");
    return CPE_OK;
}

extern "C" int32_t cpe_frame_angles_lm_batch(const double *X, const int32_t *cnt, const double *cyl_raw, const double *T,
                                             const int32_t *pose_index, int32_t G, int32_t n, double radius, const CpeFitParams *params,
                                             const double *a0_in, double *angles0, double *angles, double *fvals, int32_t *iters,
                                             double *TAGVcyl, double *Tcyl, int32_t *status, void *stream)
{
    CPE_CHECK_ARG(G >= 0 && n >= 0, "cpe_frame_angles_lm_batch: G < 0 or n < 0");
    CpeFitParams p = {1e-5, 1e-5, 100000, 100000, CPE_FIT_LM, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.tol_x >= 0 && p.tol_f >= 0 && p.max_iter > 0, "cpe_frame_angles_lm_batch: bad CpeFitParams");
    CPE_CHECK_ARG(p.mode == CPE_FIT_LM, "cpe_frame_angles_lm_batch: mode %d (the angle solver is Levenberg-Marquardt only)", p.mode);
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(X && cnt && T && angles0 && angles && fvals && iters && status, "cpe_frame_angles_lm_batch: null pointer");
    CPE_CHECK_ARG(cyl_raw || a0_in, "cpe_frame_angles_lm_batch: cyl_raw may be NULL only beside a0_in");
    CPE_LAUNCH_BEGIN();
    const AnglesOut out{angles0, angles, fvals, iters, TAGVcyl, Tcyl, status};
    CPE_KLAUNCH(k_frame_angles_lm, dim3(n), dim3(64), 0, (hipStream_t)stream, X, cnt, cyl_raw, T, pose_index, G, radius, p.tol_x, p.tol_f,
                p.max_iter, a0_in, out);
    CPE_CHECK_LAUNCH("k_frame_angles_lm");
    return CPE_OK;
}

// ---- BUILD-DEFINED (nothing like it in the reference): a grid-index shift between the two images of a frame -----------
// The selectors join the tables on equal (col,row); a detector that numbers one image a column or a row off leaves pairs
// that still meet the epipolar test (a column shift moves the partner along the epipolar line) at a wrong depth.  The one
// prior that can tell is the radius: for every candidate shift (dc, dr) of table 1, join, triangulate, keep err < th, fit a
// cylinder of the known radius (fit_init + hyp_iters of fit_lm) and count the kept points within tau of its surface.
// k_match_prepare : one wavefront per frame: counts, the refusals of k_select_triangulate, the dense table of image 2.
// k_match_score   : one wavefront per (frame, candidate); kept points compacted into LDS in join order.  The LDS of a
//                   workgroup is 32 bytes per point of table 1, so the call launches the kernel once per size class
//                   (MATCH_TIERS) and a workgroup whose frame belongs to another class leaves at once: the counts are on
//                   the device, and the host does not wait for them.
// k_match_pick    : one wavefront per frame: winner by the key (-score, |dc|+|dr|, |dc|, dc, dr), flags, id1 + offset.
namespace {
constexpr int MATCH_HDR = 8;                       // ints per frame: ok, cmin, rmin, tw, th, n1 (0 where nothing can pair), n2
constexpr int MATCH_TIERS[] = {256, 1024, MAXP};   // points of table 1 a workgroup of each launch has LDS for
constexpr int MATCH_NTIERS = 3;

__host__ __device__ constexpr size_t match_stride(int ncand) { return (size_t)MATCH_HDR + 2 * (size_t)ncand + (size_t)TBL * TBL; }

__global__ __launch_bounds__(64) void k_match_prepare(const int *__restrict__ id1, const int *__restrict__ cnt1,
                                                      const int *__restrict__ id2, const int *__restrict__ cnt2, int ncand,
                                                      int *__restrict__ ws)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int *i1 = id1 + (size_t)f * MAXP * 2, *i2 = id2 + (size_t)f * MAXP * 2;
    const int n1 = min(max(cnt1[f], 0), MAXP), n2 = min(max(cnt2[f], 0), MAXP);
    int *hdr = ws + (size_t)f * match_stride(ncand), *tb = hdr + MATCH_HDR + 2 * ncand;
    int cmin = INT_MAX, cmax = INT_MIN, rmin = INT_MAX, rmax = INT_MIN, lo = INT_MAX, hi = INT_MIN;
    for (int i = lane; i < n2; i += 64) {
        int c = i2[2 * i], r = i2[2 * i + 1];
        cmin = min(cmin, c); cmax = max(cmax, c); rmin = min(rmin, r); rmax = max(rmax, r);
    }
    for (int i = lane; i < n1; i += 64) {
        int c = i1[2 * i], r = i1[2 * i + 1];
        lo = min(lo, min(c, r)); hi = max(hi, max(c, r));
    }
    cmin = wave_min_i(cmin); cmax = wave_max_i(cmax); rmin = wave_min_i(rmin); rmax = wave_max_i(rmax);
    lo = wave_min_i(min(lo, min(cmin, rmin))); hi = wave_max_i(max(hi, max(cmax, rmax)));
    const bool pairs = n1 > 0 && n2 > 0;
    const bool ok = !(pairs && ((long long)cmax - cmin >= TBL || (long long)rmax - rmin >= TBL || lo < -9999 || hi > 9999));
    const int tw = (pairs && ok) ? cmax - cmin + 1 : 0, thh = (pairs && ok) ? rmax - rmin + 1 : 0;
    if (lane == 0) {
        hdr[0] = ok ? 1 : 0; hdr[1] = cmin; hdr[2] = rmin; hdr[3] = tw; hdr[4] = thh;
        hdr[5] = (pairs && ok) ? n1 : 0; hdr[6] = n2; hdr[7] = 0;
    }
    for (int i = lane; i < tw * thh; i += 64) tb[i] = INT_MAX;
    __syncthreads();
    if (pairs && ok)
        for (int i = lane; i < n2; i += 64) atomicMin(&tb[(i2[2 * i + 1] - rmin) * tw + (i2[2 * i] - cmin)], i);
}

__global__ __launch_bounds__(64) void k_match_score(const double *__restrict__ xy1, const int *__restrict__ id1,
                                                    const double *__restrict__ xy2, const double *__restrict__ K1,
                                                    const double *__restrict__ K2, const double *__restrict__ T21, int win_c,
                                                    int win_r, double R, double th, double tau, int hyp_iters, int cap_lo,
                                                    int cap_hi, int *__restrict__ ws)
{
    const int nr = 2 * win_r + 1, ncand = (2 * win_c + 1) * nr;
    const int f = blockIdx.x / ncand, cand = blockIdx.x - f * ncand, lane = threadIdx.x;
    int *hdr = ws + (size_t)f * match_stride(ncand);
    const int n1 = hdr[5];
    if (n1 <= cap_lo || n1 > cap_hi) return;       // another launch has the LDS this frame needs
    double *sP = fit_dyn, *sD = fit_dyn + (size_t)cap_hi * 3;   // dynamic LDS: cap_hi * 4 doubles
    __shared__ int sNb[20];
    const int dc = cand / nr - win_c, dr = cand - (cand / nr) * nr - win_r;
    const int cmin = hdr[1], rmin = hdr[2], tw = hdr[3], thh = hdr[4];
    const int *tb = hdr + MATCH_HDR + 2 * ncand;
    const double *a1 = xy1 + (size_t)f * MAXP * 2, *a2 = xy2 + (size_t)f * MAXP * 2;
    const int *i1 = id1 + (size_t)f * MAXP * 2;
    int m = 0, score = 0;
    if (n1 > 0) {
        double P1[12], P2[12];
        {
            const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            double k1[9], k2[9], tt[16];
            for (int k = 0; k < 9; k++) { k1[k] = K1[k]; k2[k] = K2[k]; }
            for (int k = 0; k < 16; k++) tt[k] = T21[k];
            make_P(k1, I4, P1);
            make_P(k2, tt, P2);
        }
        // join in image-1 order (first occurrence in image 2): the pairs (i, j) go to LDS first, so that the DLT rounds below
        // have every lane at work (a shifted table 1 finds partners for only a part of its rows).  They lie where fit_init
        // keeps its distances later: 2 ints = 1 double per point
        int *sIJ = reinterpret_cast<int *>(sD);
        int nj = 0;
        for (int i0 = 0; i0 < n1; i0 += 64) {
            const int i = i0 + lane;
            int j = INT_MAX;
            if (i < n1) {
                const int c = i1[2 * i] + dc - cmin, r = i1[2 * i + 1] + dr - rmin;
                if (c >= 0 && c < tw && r >= 0 && r < thh) j = tb[r * tw + c];
            }
            const unsigned long long b = __ballot(j != INT_MAX);
            if (j != INT_MAX) {
                const int pos = nj + __popcll(b & ((1ull << lane) - 1ull));     // pos < n1 <= cap_hi
                sIJ[2 * pos] = i; sIJ[2 * pos + 1] = j;
            }
            nj += __popcll(b);
        }
        __syncthreads();
        // DLT of every pair, err < th, compaction in join order
        for (int k0 = 0; k0 < nj; k0 += 64) {
            const int k = k0 + lane;
            bool take = false;
            double X[3] = {0, 0, 0};
            if (k < nj) {
                const int i = sIJ[2 * k], j = sIJ[2 * k + 1];
                double e;
                triangulate_one(P1, P2, a1[2 * i], a1[2 * i + 1], a2[2 * j], a2[2 * j + 1], X, e);
                take = e < th;
            }
            const unsigned long long b = __ballot(take);
            if (take) {
                const int pos = m + __popcll(b & ((1ull << lane) - 1ull));   // pos < nj <= cap_hi
                sP[3 * pos] = X[0]; sP[3 * pos + 1] = X[1]; sP[3 * pos + 2] = X[2];
            }
            m += __popcll(b);
        }
        __syncthreads();
        if (m >= CPE_FIT_MIN_POINTS) {
            double x0[6], f0, xf[6], ffinal;
            int it, ev;
            fit_init(sP, m, R, lane, sD, sNb, x0, f0);
            if (fit_finite(x0, f0)) {
                fit_lm(sP, m, R, lane, 1e-5, 1e-5, hyp_iters, x0, f0, xf, ffinal, it, ev);
                if (fit_finite(xf, ffinal)) {
                    int c = 0;
                    for (int k = lane; k < m; k += 64) c += ransac_inlier(sP, k, xf, R, tau) ? 1 : 0;
                    score = wave_sum_i(c);
                }
            }
        }
    }
    if (lane == 0) { hdr[MATCH_HDR + cand] = score; hdr[MATCH_HDR + ncand + cand] = m; }
}

__global__ __launch_bounds__(64) void k_match_pick(const int *__restrict__ id1, const int *__restrict__ cnt1, int win_c, int win_r,
                                                   int min_score, const int *__restrict__ ws, int *__restrict__ o_offset,
                                                   int *__restrict__ o_score, int *__restrict__ o_scores, int *__restrict__ o_flags,
                                                   int *__restrict__ o_id1)
{
    const int nr = 2 * win_r + 1, ncand = (2 * win_c + 1) * nr;
    const int f = blockIdx.x, lane = threadIdx.x;
    const int *hdr = ws + (size_t)f * match_stride(ncand), *sc = hdr + MATCH_HDR, *kept = sc + ncand;
    // smallest key (-score, |dc|+|dr|, |dc|, dc, dr) as one integer: (0,0) wins every tie it is part of
    unsigned long long best = ~0ull;
    for (int k = lane; k < ncand; k += 64) {
        const int dc = k / nr - win_c, dr = k - (k / nr) * nr - win_r;
        const unsigned long long key = ((unsigned long long)(MAXP - sc[k]) << 48) | ((unsigned long long)(abs(dc) + abs(dr)) << 40) |
                                       ((unsigned long long)abs(dc) << 32) | ((unsigned long long)(dc + CPE_MATCH_MAX_WIN) << 24) |
                                       ((unsigned long long)(dr + CPE_MATCH_MAX_WIN) << 16) | (unsigned long long)k;
        best = key < best ? key : best;
        if (o_scores) o_scores[(size_t)f * ncand + k] = sc[k];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
    }
    const int win = (int)(best & 0xffffull);
    int second = 0;                                // the second-largest value among all candidates (0 with one candidate)
    for (int k = lane; k < ncand; k += 64)
        if (k != win) second = max(second, sc[k]);
    second = wave_max_i(second);
    const int wdc = win / nr - win_c, wdr = win - (win / nr) * nr - win_r, top = sc[win];
    int flags = 0, dc = wdc, dr = wdr;
    if (!hdr[0]) flags |= CPE_MATCH_FLAG_OVERFLOW;
    if (top < min_score) { flags |= CPE_MATCH_FLAG_WEAK; dc = 0; dr = 0; }
    if ((win_c > 0 && abs(wdc) == win_c) || (win_r > 0 && abs(wdr) == win_r)) flags |= CPE_MATCH_FLAG_EDGE;
    if (dc != 0 || dr != 0) flags |= CPE_MATCH_FLAG_SHIFTED;
    if (lane == 0) {
        o_offset[2 * f] = dc; o_offset[2 * f + 1] = dr;
        o_score[4 * f] = top; o_score[4 * f + 1] = second; o_score[4 * f + 2] = sc[win_c * nr + win_r]; o_score[4 * f + 3] = kept[win];
        o_flags[f] = flags;
    }
    const int n1 = min(max(cnt1[f], 0), MAXP);
    const int *i1 = id1 + (size_t)f * MAXP * 2;
    int *o1 = o_id1 + (size_t)f * MAXP * 2;
    for (int i = lane; i < n1; i += 64) { o1[2 * i] = i1[2 * i] + dc; o1[2 * i + 1] = i1[2 * i + 1] + dr; }
}
}  // namespace

extern "C" size_t cpe_match_offset_workspace_bytes(int32_t n, int32_t win_c, int32_t win_r)
{
    if (n <= 0 || win_c < 0 || win_r < 0 || win_c > CPE_MATCH_MAX_WIN || win_r > CPE_MATCH_MAX_WIN) return 0;
    return (size_t)n * match_stride((2 * win_c + 1) * (2 * win_r + 1)) * sizeof(int);
}

extern "C" int32_t cpe_match_offset_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                          const int32_t *id2, const int32_t *cnt2, int32_t n, const double *K1, const double *K2,
                                          const double *T21, double radius, const CpeMatchParams *params, void *ws, size_t ws_bytes,
                                          int32_t *offset, int32_t *score, int32_t *scores, int32_t *flags, int32_t *id1_out,
                                          void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_match_offset_batch: n < 0");
    CpeMatchParams p = {4, 4, 0.3, 0.5, 8, 8};
    if (params) p = *params;
    CPE_CHECK_ARG(p.win_c >= 0 && p.win_c <= CPE_MATCH_MAX_WIN && p.win_r >= 0 && p.win_r <= CPE_MATCH_MAX_WIN,
                  "cpe_match_offset_batch: window must be 0..%d in both directions", CPE_MATCH_MAX_WIN);
    CPE_CHECK_ARG(p.th > 0 && p.tau > 0 && p.hyp_iters >= 1 && p.hyp_iters <= 200 && p.min_score >= 0,
                  "cpe_match_offset_batch: bad CpeMatchParams (th > 0, tau > 0, hyp_iters 1..200, min_score >= 0)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(xy1 && id1 && cnt1 && xy2 && id2 && cnt2 && K1 && K2 && T21 && offset && score && flags && id1_out,
                  "cpe_match_offset_batch: null pointer");
    CPE_CHECK_ARG(id1_out != id1, "cpe_match_offset_batch: id1_out may not be id1");
    const int ncand = (2 * p.win_c + 1) * (2 * p.win_r + 1);
    CPE_CHECK_ARG((long long)n * ncand <= INT_MAX, "cpe_match_offset_batch: n * candidates exceeds 2^31 - 1");
    if (!ws || ws_bytes < cpe_match_offset_workspace_bytes(n, p.win_c, p.win_r)) {
        cpe::set_error("cpe_match_offset_batch: workspace too small (%zu < %zu)", ws_bytes,
                       cpe_match_offset_workspace_bytes(n, p.win_c, p.win_r));
        return CPE_ERR_WORKSPACE;
    }
    CPE_LAUNCH_BEGIN();
    CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_match_score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FIT_LDS_BYTES));
    CPE_KLAUNCH(k_match_prepare, dim3(n), dim3(64), 0, (hipStream_t)stream, id1, cnt1, id2, cnt2, ncand, (int *)ws);
    CPE_CHECK_LAUNCH("k_match_prepare");
    for (int t = 0; t < MATCH_NTIERS; t++) {
        const int cap_lo = t == 0 ? -1 : MATCH_TIERS[t - 1], cap_hi = MATCH_TIERS[t];
        CPE_KLAUNCH(k_match_score, dim3(n * ncand), dim3(64), (size_t)cap_hi * 4 * sizeof(double), (hipStream_t)stream, xy1, id1, xy2, K1, K2,
                    T21, p.win_c, p.win_r, radius, p.th, p.tau, p.hyp_iters, cap_lo, cap_hi, (int *)ws);
        CPE_CHECK_LAUNCH("k_match_score");
    }
    CPE_KLAUNCH(k_match_pick, dim3(n), dim3(64), 0, (hipStream_t)stream, id1, cnt1, p.win_c, p.win_r, p.min_score, (const int *)ws, offset,
                score, scores, flags, id1_out);
    CPE_CHECK_LAUNCH("k_match_pick");
    return CPE_OK;
}

// ------------------------------------------------------------------------------------------ planar target
// BUILD-DEFINED (include/cpe.h cpe_fit_plane_batch, cpe_index_planes_batch): fitplane.m:1-16 per frame with an optional
// trimming loop, the affine grid map, the board pose; and the laser planes over several board poses with their common point.
// The points are read from global memory in every pass (a frame's table is at most 48 KB and stays in L2); lane l takes points
// l, l + 64, ... and the sums go through wave_sum, as everywhere in this file.
namespace {

__device__ __forceinline__ bool finite3(const double *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the moments a plane fit starts from
struct PlaneMoments {
    double c[3], w[3], V[9];   // centroid, eigenvalues ascending, eigenvectors (columns)
    int N;
};

// enough points, and not collinear or coincident: lambda_mid > 1e-12 lambda_max
__device__ __forceinline__ bool plane_spread_ok(const PlaneMoments &m) { return m.N >= 3 && m.w[1] > 1e-12 * m.w[2]; }

// the sums of plane_moments: the count Np, the centroid c, then in a second pass the centred scatter q = xx xy xz yy yz zz
template <class Each>
__device__ __forceinline__ void plane_sums(Each each, int &Np, double *c, double *q)
{
    double s[3] = {0, 0, 0};
    int cn = 0;
    each([&](const double *p) { s[0] = s[0] + p[0]; s[1] = s[1] + p[1]; s[2] = s[2] + p[2]; cn++; });
    Np = wave_sum_i(cn);
    const double N = (double)(Np > 0 ? Np : 1);
#pragma unroll
    for (int a = 0; a < 3; a++) c[a] = wave_sum(s[a]) / N;
#pragma unroll
    for (int a = 0; a < 6; a++) q[a] = 0;
    const double c0 = c[0], c1 = c[1], c2 = c[2];
    each([&](const double *p) {
        const double e0 = p[0] - c0, e1 = p[1] - c1, e2 = p[2] - c2;
        q[0] = q[0] + e0 * e0; q[1] = q[1] + e0 * e1; q[2] = q[2] + e0 * e2;
        q[3] = q[3] + e1 * e1; q[4] = q[4] + e1 * e2; q[5] = q[5] + e2 * e2;
    });
#pragma unroll
    for (int a = 0; a < 6; a++) q[a] = wave_sum(q[a]);
}

// centroid, then the centred covariance / (N - 1) in a second pass, then its eigen-decomposition (wave-uniform results; the normal
// of fitplane.m is V(:,1)).  `each(body)` calls body(p) for every point p[3] of the set that this lane takes; it is walked twice
template <class Each>
__device__ __forceinline__ void plane_moments(Each each, PlaneMoments &m)
{
    double q[6];
    plane_sums(each, m.N, m.c, q);
    const double d = (double)(m.N > 1 ? m.N - 1 : 1);
#pragma unroll
    for (int a = 0; a < 6; a++) q[a] = q[a] / d;
    const double Cv[9] = {q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]};
    eig3(Cv, m.w, m.V);
}

__global__ __launch_bounds__(64) void k_fit_plane(const double *__restrict__ X, const int *__restrict__ idx, const int *__restrict__ cnt,
                                                  double tau, int max_rounds, double *__restrict__ o_P, double *__restrict__ o_T,
                                                  double *__restrict__ o_grid, double *__restrict__ o_stats, int *__restrict__ o_ninl,
                                                  uint8_t *__restrict__ o_mask, int *__restrict__ o_flags, int *__restrict__ o_status)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(cnt[f], 0), MAXP);
    const double *Xf = X + (size_t)f * MAXP * 3;
    const int *If = idx + (size_t)f * MAXP * 2;
    // the mask of the current fit lives in the output: slot k is written and read by lane k % 64 only
    uint8_t *mk = o_mask + (size_t)f * MAXP;
    for (int k = lane; k < MAXP; k += 64) mk[k] = (k < n && finite3(Xf + 3 * k)) ? 1 : 0;
    auto each = [&](auto body) {
        for (int k = lane; k < n; k += 64)
            if (mk[k]) body(Xf + 3 * k);
    };
    PlaneMoments m;
    double nrm[3], P4 = 0;
    int refits = 0;
    bool ok;
    for (;;) {
        plane_moments(each, m);
        ok = plane_spread_ok(m);
        if (!ok) break;
        nrm[0] = m.V[0]; nrm[1] = m.V[3]; nrm[2] = m.V[6];
        const bool flip = nrm[2] < 0 || (nrm[2] == 0 && (nrm[1] < 0 || (nrm[1] == 0 && nrm[0] < 0)));
        if (flip) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
        P4 = -((nrm[0] * m.c[0] + nrm[1] * m.c[1]) + nrm[2] * m.c[2]);
        if (!(tau > 0) || refits >= max_rounds) break;
        int changed = 0;
        for (int k = lane; k < n; k += 64) {
            const double *p = Xf + 3 * k;
            const uint8_t in = (finite3(p) && fabs(((nrm[0] * p[0] + nrm[1] * p[1]) + nrm[2] * p[2]) + P4) < tau) ? 1 : 0;
            changed += in != mk[k];
            mk[k] = in;
        }
        if (wave_sum_i(changed) == 0) break;
        refits++;
    }
    if (!ok) {
        for (int k = lane; k < n; k += 64) mk[k] = 0;
        if (lane < 4) o_P[(size_t)f * 4 + lane] = 0;
        if (lane < 16) o_T[(size_t)f * 16 + lane] = 0;
        if (lane < 9) o_grid[(size_t)f * 9 + lane] = 0;
        if (lane < 8) o_stats[(size_t)f * 8 + lane] = 0;
        if (lane == 0) { o_ninl[f] = 0; o_flags[f] = 0; o_status[f] = CPE_ST_FEW_POINTS; }
        return;
    }
    // residuals, index moments, the first point with index (0,0)
    double r2 = 0, rmax = 0, sa = 0, sb = 0;
    int first0 = INT_MAX;
    for (int k = lane; k < n; k += 64) {
        if (!mk[k]) continue;
        const double *p = Xf + 3 * k;
        const double r = fabs(((nrm[0] * p[0] + nrm[1] * p[1]) + nrm[2] * p[2]) + P4);
        r2 = r2 + r * r;
        rmax = fmax(rmax, r);
        const int a = If[2 * k], b = If[2 * k + 1];
        sa = sa + (double)a; sb = sb + (double)b;
        if (a == 0 && b == 0) first0 = min(first0, k);
    }
    const double N = (double)m.N;
    r2 = wave_sum(r2);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
    const double ma = wave_sum(sa) / N, mb = wave_sum(sb) / N;
    first0 = wave_min_i(first0);
    // normal equations of X - c ~ (a - ma) U + (b - mb) V
    double g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // Saa Sab Sbb | Sa.x[3] | Sb.x[3]
    for (int k = lane; k < n; k += 64) {
        if (!mk[k]) continue;
        const double *p = Xf + 3 * k;
        const double da = (double)If[2 * k] - ma, db = (double)If[2 * k + 1] - mb;
        const double e0 = p[0] - m.c[0], e1 = p[1] - m.c[1], e2 = p[2] - m.c[2];
        g[0] = g[0] + da * da; g[1] = g[1] + da * db; g[2] = g[2] + db * db;
        g[3] = g[3] + da * e0; g[4] = g[4] + da * e1; g[5] = g[5] + da * e2;
        g[6] = g[6] + db * e0; g[7] = g[7] + db * e1; g[8] = g[8] + db * e2;
    }
#pragma unroll
    for (int a = 0; a < 9; a++) g[a] = wave_sum(g[a]);
    int flags = 0;
    double UV[6] = {0, 0, 0, 0, 0, 0}, O[3] = {0, 0, 0}, grms = 0;
    if (g[0] * g[2] - g[1] * g[1] <= 1e-12 * (g[0] * g[2])) flags |= CPE_PLANEFIT_NO_GRID;
    else {
        double M[4] = {g[0], g[1], g[1], g[2]}, rhs[6] = {g[3], g[4], g[5], g[6], g[7], g[8]};
        gauss_solve<2, 3>(M, rhs, UV);
#pragma unroll
        for (int a = 0; a < 3; a++) O[a] = m.c[a] - (ma * UV[a] + mb * UV[3 + a]);
        double e = 0;
        for (int k = lane; k < n; k += 64) {
            if (!mk[k]) continue;
            const double *p = Xf + 3 * k;
            const double a = (double)If[2 * k], b = (double)If[2 * k + 1];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double d = p[c] - ((O[c] + a * UV[c]) + b * UV[3 + c]);
                e = e + d * d;
            }
        }
        grms = sqrt(wave_sum(e) / N);
    }
    // pose
    double ux[3] = {1, 0, 0};
    if (!(flags & CPE_PLANEFIT_NO_GRID)) { ux[0] = UV[0]; ux[1] = UV[1]; ux[2] = UV[2]; }
    double xa[3], xn;
    {
        const double un = (ux[0] * nrm[0] + ux[1] * nrm[1]) + ux[2] * nrm[2];
#pragma unroll
        for (int a = 0; a < 3; a++) xa[a] = ux[a] - un * nrm[a];
        xn = sqrt((xa[0] * xa[0] + xa[1] * xa[1]) + xa[2] * xa[2]);
    }
    if (!(xn > 0) || !isfinite(xn)) {
        const double un = nrm[1];
        xa[0] = 0 - un * nrm[0]; xa[1] = 1 - un * nrm[1]; xa[2] = 0 - un * nrm[2];
        xn = sqrt((xa[0] * xa[0] + xa[1] * xa[1]) + xa[2] * xa[2]);
    }
#pragma unroll
    for (int a = 0; a < 3; a++) xa[a] = xa[a] / xn;
    const double ya[3] = {nrm[1] * xa[2] - nrm[2] * xa[1], nrm[2] * xa[0] - nrm[0] * xa[2], nrm[0] * xa[1] - nrm[1] * xa[0]};
    double org[3] = {m.c[0], m.c[1], m.c[2]};
    if (first0 != INT_MAX) {
        flags |= CPE_PLANEFIT_ORIGIN_POINT;
        org[0] = Xf[3 * first0]; org[1] = Xf[3 * first0 + 1]; org[2] = Xf[3 * first0 + 2];
    } else if (!(flags & CPE_PLANEFIT_NO_GRID)) {
        org[0] = O[0]; org[1] = O[1]; org[2] = O[2];
    }
    {
        const double d = ((nrm[0] * org[0] + nrm[1] * org[1]) + nrm[2] * org[2]) + P4;
#pragma unroll
        for (int a = 0; a < 3; a++) org[a] = org[a] - d * nrm[a];
    }
    if (lane == 0) {
        double *P = o_P + (size_t)f * 4, *T = o_T + (size_t)f * 16, *G = o_grid + (size_t)f * 9, *S = o_stats + (size_t)f * 8;
        P[0] = nrm[0]; P[1] = nrm[1]; P[2] = nrm[2]; P[3] = P4;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            T[a * 4 + 0] = xa[a]; T[a * 4 + 1] = ya[a]; T[a * 4 + 2] = nrm[a]; T[a * 4 + 3] = org[a];
            G[a] = O[a]; G[3 + a] = UV[a]; G[6 + a] = UV[3 + a];
            S[2 + a] = m.w[a];
        }
        T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
        S[0] = sqrt(r2 / N); S[1] = rmax; S[5] = grms; S[6] = (double)refits; S[7] = 0;
        o_ninl[f] = m.N; o_flags[f] = flags; o_status[f] = CPE_ST_OK;
    }
}

__global__ __launch_bounds__(64) void k_index_planes(const double *__restrict__ X, const int *__restrict__ idx, const int *__restrict__ cnt,
                                                     int n, const uint8_t *__restrict__ use, const int *__restrict__ frame_ok, int lo, int L,
                                                     double min_spread, double *__restrict__ o_P, double *__restrict__ o_stats,
                                                     int *__restrict__ o_count, int *__restrict__ o_frames, int *__restrict__ o_status)
{
    const int line = blockIdx.x, lane = threadIdx.x;   // line = family * L + (v - lo)
    const int fam = line / L, v = lo + (line - fam * L);
    int frames = 0;
    bool count_frames = true;
    auto each = [&](auto body) {
        for (int f = 0; f < n; f++) {
            if (frame_ok && frame_ok[f] == 0) continue;
            const int c = min(max(cnt[f], 0), MAXP);
            const size_t base = (size_t)f * MAXP;
            bool any = false;
            for (int k = lane; k < c; k += 64) {
                if (idx[(base + k) * 2 + fam] != v) continue;
                if (use && use[base + k] == 0) continue;
                const double *p = X + (base + k) * 3;
                if (!finite3(p)) continue;
                body(p);
                any = true;
            }
            if (count_frames && __ballot(any) != 0ull) frames++;
        }
        count_frames = false;
    };
    PlaneMoments m;
    plane_moments(each, m);
    bool ok = m.N >= 3 && frames >= 2 && m.w[2] > 0;
    const double spread = ok ? m.w[1] / m.w[2] : 0.0;
    ok = ok && !(spread < min_spread);
    double nrm[3] = {m.V[0], m.V[3], m.V[6]}, P4 = 0, r2 = 0, rmax = 0;
    if (ok) {
        const double a0 = fabs(nrm[0]), a1 = fabs(nrm[1]), a2 = fabs(nrm[2]);
        const double big = (a0 >= a1 && a0 >= a2) ? nrm[0] : (a1 >= a2 ? nrm[1] : nrm[2]);
        if (big < 0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
        P4 = -((nrm[0] * m.c[0] + nrm[1] * m.c[1]) + nrm[2] * m.c[2]);
        each([&](const double *p) {
            const double r = fabs(((nrm[0] * p[0] + nrm[1] * p[1]) + nrm[2] * p[2]) + P4);
            r2 = r2 + r * r;
            rmax = fmax(rmax, r);
        });
        r2 = wave_sum(r2);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
    }
    if (lane == 0) {
        double *P = o_P + (size_t)line * 4, *S = o_stats + (size_t)line * 4;
        P[0] = ok ? nrm[0] : 0.0; P[1] = ok ? nrm[1] : 0.0; P[2] = ok ? nrm[2] : 0.0; P[3] = ok ? P4 : 0.0;
        S[0] = ok ? sqrt(r2 / (double)m.N) : 0.0; S[1] = ok ? rmax : 0.0; S[2] = ok ? spread : 0.0; S[3] = 0;
        o_count[line] = m.N; o_frames[line] = frames; o_status[line] = ok ? CPE_ST_OK : CPE_ST_FEW_POINTS;
    }
}

// the point nearest to all OK planes: (sum n n') C = -sum n P4
__global__ __launch_bounds__(64) void k_planes_centre(const double *__restrict__ P, const int *__restrict__ status, int L,
                                                      double *__restrict__ o_centre, int *__restrict__ o_status)
{
    const int lane = threadIdx.x;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int ok0 = 0, ok1 = 0;
    for (int i = lane; i < 2 * L; i += 64) {
        if (status[i] != CPE_ST_OK) continue;
        const double j[3] = {P[4 * i], P[4 * i + 1], P[4 * i + 2]};
        normal_accumulate<3>(j, P[4 * i + 3], acc);
        if (i < L) ok0++; else ok1++;
    }
#pragma unroll
    for (int a = 0; a < 9; a++) acc[a] = wave_sum(acc[a]);
    ok0 = wave_sum_i(ok0); ok1 = wave_sum_i(ok1);
    double M[9] = {acc[0], acc[1], acc[2], acc[1], acc[3], acc[4], acc[2], acc[4], acc[5]};
    double rhs[3] = {-acc[6], -acc[7], -acc[8]}, Cc[3] = {0, 0, 0};
    bool ok = gauss_solve<3>(M, rhs, Cc);
    ok = ok && ok0 >= 2 && ok1 >= 2 && finite3(Cc);
    double e = 0;
    if (ok)
        for (int i = lane; i < 2 * L; i += 64) {
            if (status[i] != CPE_ST_OK) continue;
            const double r = ((P[4 * i] * Cc[0] + P[4 * i + 1] * Cc[1]) + P[4 * i + 2] * Cc[2]) + P[4 * i + 3];
            e = e + r * r;
        }
    e = wave_sum(e);
    if (lane == 0) {
        o_centre[0] = ok ? Cc[0] : 0.0; o_centre[1] = ok ? Cc[1] : 0.0; o_centre[2] = ok ? Cc[2] : 0.0;
        o_centre[3] = ok ? sqrt(e / (double)(ok0 + ok1)) : 0.0;
        o_status[0] = ok ? CPE_ST_OK : CPE_ST_FEW_POINTS;
    }
}

// The one-camera rule of include/cpe.h cpe_table_triangulate_batch in pieces, shared by k_table_triangulate and
// k_fused_triangulate: the same source lines, so the same bits.
struct TriCam {
    double R[9], o[3];              // rotation (rows) of Tc and the camera centre in camera-1 coordinates
    double k0, k1, k2, k4, k5;
};

// R, t of Tc, the identity without one: the same arithmetic either way
__device__ __forceinline__ void tri_cam(const double *__restrict__ K, const double *__restrict__ Tc, TriCam &c)
{
    double t[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 9; a++) c.R[a] = (a % 4 == 0) ? 1.0 : 0.0;
    if (Tc) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            c.R[3 * r] = Tc[4 * r]; c.R[3 * r + 1] = Tc[4 * r + 1]; c.R[3 * r + 2] = Tc[4 * r + 2];
            t[r] = Tc[4 * r + 3];
        }
    }
    c.k0 = K[0]; c.k1 = K[1]; c.k2 = K[2]; c.k4 = K[4]; c.k5 = K[5];
#pragma unroll
    for (int a = 0; a < 3; a++) c.o[a] = -((c.R[a] * t[0] + c.R[3 + a] * t[1]) + c.R[6 + a] * t[2]);
}

// step 2: the unit ray of pixel (x, y) in camera-1 coordinates
__device__ __forceinline__ void tri_ray(const TriCam &c, double x, double y, double *d)
{
    const double vy = (y - c.k5) / c.k4;
    const double vx = ((x - c.k2) - c.k1 * vy) / c.k0;
#pragma unroll
    for (int a = 0; a < 3; a++) d[a] = (c.R[a] * vx + c.R[3 + a] * vy) + c.R[6 + a];
    const double dn = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int a = 0; a < 3; a++) d[a] = d[a] / dn;
}

// step 3: the usable planes of the indices v[2] -> bits; pl[c] is loaded for a set bit only
__device__ __forceinline__ int tri_planes(const double *__restrict__ P, const int *__restrict__ line_status, int lo, int hi, int L, int swap,
                                          const int *v, double (*pl)[4])
{
    int used = 0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int fam = c ^ swap;
        if (v[c] < lo || v[c] > hi) continue;                              // (compared, not subtracted: v may be any int)
        const int line = fam * L + (v[c] - lo);
        if (line_status[line] != CPE_ST_OK) continue;
#pragma unroll
        for (int a = 0; a < 4; a++) pl[c][a] = P[(size_t)line * 4 + a];
        used |= 1 << c;
    }
    return used;
}

// steps 4 - 7 for the ray (o, d) and the planes of `used`: -> accepted; early: refused in steps 1 / 4 / 5, otherwise in 6 / 7.
// X and rs are written for an accepted point; rs of an unused plane stays as the caller set it
__device__ __forceinline__ bool tri_cut(const double *o, const double *d, const double (*pl)[4], int used, bool pixel_ok, int need_both,
                                        double min_sin2, double max_res, double *X, double *rs, bool &early)
{
    double den = 0, sab = 0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (!(used & (1 << c))) continue;
        const double a_k = (pl[c][0] * d[0] + pl[c][1] * d[1]) + pl[c][2] * d[2];
        const double b_k = ((pl[c][0] * o[0] + pl[c][1] * o[1]) + pl[c][2] * o[2]) + pl[c][3];
        den = den + a_k * a_k;
        sab = sab + a_k * b_k;
    }
    early = !pixel_ok || used == 0 || (need_both && used != 3) || den < min_sin2 || !isfinite(den);
    if (early) return false;
    const double s = -sab / den;
    bool acc = s > 0 && isfinite(s);
    if (acc) {
#pragma unroll
        for (int a = 0; a < 3; a++) X[a] = o[a] + s * d[a];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (!(used & (1 << c))) continue;
            rs[c] = ((pl[c][0] * X[0] + pl[c][1] * X[1]) + pl[c][2] * X[2]) + pl[c][3];
            if (max_res > 0 && fabs(rs[c]) > max_res) acc = false;
        }
    }
    return acc;
}

// 3-D points from one camera and the laser-plane table (include/cpe.h cpe_table_triangulate_batch, whose numbered rule this
// follows).  One lane per point, rounds of 64; the accepted points keep their table order: a ballot, the popcount of the lanes
// below, and the base of the round carried on.  The table (at most 2 x 256 planes, 18 KB with the statuses) is read where a point
// needs it: a frame of a few hundred points touches about as many bytes as a copy into LDS would, and every frame shares it in L2.
__global__ __launch_bounds__(64) void k_table_triangulate(const double *__restrict__ xy, const int *__restrict__ id, const int *__restrict__ cnt,
                                                          const double *__restrict__ K, const double *__restrict__ Tc,
                                                          const double *__restrict__ P, const int *__restrict__ line_status, int lo, int hi,
                                                          int swap, int need_both, double min_sin2, double max_res,
                                                          double *__restrict__ o_X, int *__restrict__ o_idx, double *__restrict__ o_res,
                                                          int *__restrict__ o_src, int *__restrict__ o_m, int *__restrict__ o_counts,
                                                          double *__restrict__ o_stats)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(cnt[f], 0), MAXP);
    const int L = hi - lo + 1;                     // 1..CPE_MAXL, checked by the host
    const size_t base = (size_t)f * MAXP;
    TriCam cam;
    tri_cam(K, Tc, cam);
    const unsigned long long below = (1ull << lane) - 1ull;
    int m = 0, both = 0, ref_a = 0, ref_b = 0;
    double r2 = 0, rmax = 0;
    for (int k0p = 0; k0p < n; k0p += 64) {
        const int k = k0p + lane;
        bool in = k < n, acc = false, early = false;   // early: refused in steps 1 / 4 / 5, otherwise in 6 / 7
        double X[3] = {0, 0, 0}, rs[2] = {0, 0};
        int v[2] = {0, 0}, used = 0;
        if (in) {
            const double x = xy[(base + k) * 2], y = xy[(base + k) * 2 + 1];
            v[0] = id[(base + k) * 2]; v[1] = id[(base + k) * 2 + 1];
            double d[3], pl[2][4];
            tri_ray(cam, x, y, d);
            used = tri_planes(P, line_status, lo, hi, L, swap, v, pl);
            acc = tri_cut(cam.o, d, pl, used, isfinite(x) && isfinite(y), need_both, min_sin2, max_res, X, rs, early);
        }
        const unsigned long long bal = __ballot(acc);
        ref_a += __popcll(__ballot(in && early));
        ref_b += __popcll(__ballot(in && !early && !acc));
        both += __popcll(__ballot(acc && used == 3));
        if (acc) {
            const size_t slot = base + (size_t)(m + __popcll(bal & below));       // <= base + k: inside the frame's table
            o_X[slot * 3] = X[0]; o_X[slot * 3 + 1] = X[1]; o_X[slot * 3 + 2] = X[2];
            o_idx[slot * 2] = v[0]; o_idx[slot * 2 + 1] = v[1];
            o_res[slot * 2] = rs[0]; o_res[slot * 2 + 1] = rs[1];
            o_src[slot * 2] = used; o_src[slot * 2 + 1] = k;
            r2 = r2 + (rs[0] * rs[0] + rs[1] * rs[1]);
            rmax = fmax(rmax, fmax(fabs(rs[0]), fabs(rs[1])));
        }
        m += __popcll(bal);
    }
    r2 = wave_sum(r2);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
    if (lane == 0) {
        o_m[f] = m;
        o_counts[4 * f] = m; o_counts[4 * f + 1] = both; o_counts[4 * f + 2] = ref_a; o_counts[4 * f + 3] = ref_b;
        o_stats[2 * f] = m > 0 ? sqrt(r2 / (double)(m + both)) : 0.0;
        o_stats[2 * f + 1] = m > 0 ? rmax : 0.0;
    }
}

// M += w2 (I - d d'), b += w2 (I - d d') o: a ray's part of the normal equations of "the point nearest to rays and planes"
__device__ __forceinline__ void fused_add_ray(double w2, const double *d, const double *o, double *M, double *b)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double p[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            p[c] = (r == c ? 1.0 : 0.0) - d[r] * d[c];
            M[3 * r + c] = M[3 * r + c] + w2 * p[c];
        }
        b[r] = b[r] + w2 * ((p[0] * o[0] + p[1] * o[1]) + p[2] * o[2]);
    }
}

// distance of X from the ray (o, d) in pixels: the distance times k0 / s, s the depth of X along the ray
__device__ __forceinline__ double fused_ray_res(const double *X, const double *o, const double *d, double k0)
{
    const double u0 = X[0] - o[0], u1 = X[1] - o[1], u2 = X[2] - o[2];
    const double s = (u0 * d[0] + u1 * d[1]) + u2 * d[2];
    const double p0 = u0 - s * d[0], p1 = u1 - s * d[1], p2 = u2 - s * d[2];
    return sqrt((p0 * p0 + p1 * p1) + p2 * p2) * (k0 / s);
}

// Fused 3-D points: both cameras' rays and the laser planes in one solve (include/cpe.h cpe_fused_triangulate_batch, whose
// numbered rule this follows).  One wavefront per frame.  The join goes through the dense (col,row) -> slot table of table 2,
// 16-bit slot numbers in LDS (128 x 128 x 2 = 32768 B) beside a "taken" byte per slot of table 2 (2048 B: bytes, so that lanes
// set them with plain stores): 34816 B in all.  The first occurrence of an index wins without an atomic: the rounds of table 2
// are written from the last to the first, and inside a round a lane whose slot number is below the stored one writes again
// until none is.  Then one loop of rounds of 64 candidates: the rounds of table 1 (paired or left-only), a barrier, the rounds
// of table 2 (untaken entries, right-only); compaction as in k_table_triangulate.  The planes are read through L2, as there.
constexpr int FUSED_EMPTY = 0xFFFF;
__global__ __launch_bounds__(64) void k_fused_triangulate(
    const double *__restrict__ xy1, const int *__restrict__ id1, const int *__restrict__ cnt1,
    const double *__restrict__ xy2, const int *__restrict__ id2, const int *__restrict__ cnt2,
    const double *__restrict__ K1, const double *__restrict__ K2, const double *__restrict__ T21,
    const double *__restrict__ P, const int *__restrict__ line_status, int lo, int hi, int swap, int need_both, double min_sin2,
    double sigma_px, double sigma_mm, double max_res, double max_px,
    double *__restrict__ o_X, int *__restrict__ o_idx, double *__restrict__ o_res, int *__restrict__ o_src, int *__restrict__ o_m,
    int *__restrict__ o_counts, double *__restrict__ o_stats, int *__restrict__ o_flags)
{
    __shared__ unsigned short sTbl[TBL * TBL];
    __shared__ unsigned char sTaken[MAXP];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n1 = min(max(cnt1[f], 0), MAXP), n2 = min(max(cnt2[f], 0), MAXP);
    const int L = hi - lo + 1;                     // 1..CPE_MAXL, checked by the host
    const size_t base = (size_t)f * MAXP;
    const double *a1 = xy1 + base * 2, *a2 = xy2 + base * 2;
    const int *i1 = id1 + base * 2, *i2 = id2 + base * 2;
    const bool join = n1 > 0 && n2 > 0;
    int cmin = 0, rmin = 0, tw = 0;
    if (join) {
        int cmax = INT_MIN, rmax = INT_MIN;
        cmin = INT_MAX; rmin = INT_MAX;
        for (int i = lane; i < n1; i += 64) {
            const int c = i1[2 * i], r = i1[2 * i + 1];
            cmin = min(cmin, c); cmax = max(cmax, c); rmin = min(rmin, r); rmax = max(rmax, r);
        }
        for (int i = lane; i < n2; i += 64) {
            const int c = i2[2 * i], r = i2[2 * i + 1];
            cmin = min(cmin, c); cmax = max(cmax, c); rmin = min(rmin, r); rmax = max(rmax, r);
        }
        cmin = wave_min_i(cmin); cmax = wave_max_i(cmax); rmin = wave_min_i(rmin); rmax = wave_max_i(rmax);
        if ((long long)cmax - cmin >= TBL || (long long)rmax - rmin >= TBL || cmin < -9999 || cmax > 9999 || rmin < -9999 || rmax > 9999) {
            if (lane == 0) {
                o_m[f] = 0;
#pragma unroll
                for (int a = 0; a < 6; a++) o_counts[6 * f + a] = 0;
#pragma unroll
                for (int a = 0; a < 4; a++) o_stats[4 * f + a] = 0.0;
                o_flags[f] = CPE_FIT_FLAG_OVERFLOW;
            }
            return;
        }
        tw = cmax - cmin + 1;
        const int cells = tw * (rmax - rmin + 1);                                 // <= TBL * TBL
        for (int i = lane; i < cells; i += 64) sTbl[i] = (unsigned short)FUSED_EMPTY;
        for (int i = lane; i < n2; i += 64) sTaken[i] = 0;
        __syncthreads();
        for (int k0p = ((n2 - 1) / 64) * 64; k0p >= 0; k0p -= 64) {
            const int k = k0p + lane;
            bool pend = k < n2;
            const int cell = pend ? (i2[2 * k + 1] - rmin) * tw + (i2[2 * k] - cmin) : 0;   // inside [0, cells): the range holds table 2
            while (__ballot(pend)) {
                if (pend) sTbl[cell] = (unsigned short)k;
                __syncthreads();
                if (pend) pend = (int)sTbl[cell] > k;
                __syncthreads();
            }
        }
    }
    TriCam cam1, cam2;
    tri_cam(K1, nullptr, cam1);
    tri_cam(K2, T21, cam2);
    const double wp2 = 1.0 / (sigma_mm * sigma_mm);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int rounds1 = (n1 + 63) / 64, rounds2 = (n2 + 63) / 64;
    int m = 0, n_pair = 0, n_left = 0, n_right = 0, n_ref = 0, n_trunc = 0, n_rays = 0, n_planes = 0;
    double ray2 = 0, raymax = 0, pl2 = 0, plmax = 0;
    for (int round = 0; round < rounds1 + rounds2; round++) {
        const bool second = round >= rounds1;                                     // wave-uniform: the pass over table 2
        if (round == rounds1) __syncthreads();                                    // every "taken" byte of the first pass is written
        const int k = (second ? round - rounds1 : round) * 64 + lane;
        const double *xa = second ? a2 : a1;
        const int *ia = second ? i2 : i1;
        bool cand = k < (second ? n2 : n1), acc = false;
        if (cand && second && join) cand = sTaken[k] == 0;
        double X[3] = {0, 0, 0}, rs[4] = {0, 0, 0, 0};
        int v[2] = {0, 0}, used = 0, j = -1, bits = 0;
        if (cand) {
            const double x = xa[2 * k], y = xa[2 * k + 1];
            v[0] = ia[2 * k]; v[1] = ia[2 * k + 1];
            if (!second && join) {
                const int jj = sTbl[(v[1] - rmin) * tw + (v[0] - cmin)];          // inside the table: the range holds table 1 too
                if (jj != FUSED_EMPTY) { j = jj; sTaken[j] = 1; }
            }
            TriCam cam;                                                            // wave-uniform selects, no address of either
#pragma unroll
            for (int a = 0; a < 9; a++) cam.R[a] = second ? cam2.R[a] : cam1.R[a];
#pragma unroll
            for (int a = 0; a < 3; a++) cam.o[a] = second ? cam2.o[a] : cam1.o[a];
            cam.k0 = second ? cam2.k0 : cam1.k0; cam.k1 = second ? cam2.k1 : cam1.k1; cam.k2 = second ? cam2.k2 : cam1.k2;
            cam.k4 = second ? cam2.k4 : cam1.k4; cam.k5 = second ? cam2.k5 : cam1.k5;
            double d[3], pl[2][4];
            tri_ray(cam, x, y, d);
            used = tri_planes(P, line_status, lo, hi, L, swap, v, pl);
            const bool px_ok = isfinite(x) && isfinite(y);
            if (j < 0) {
                bool early;
                acc = tri_cut(cam.o, d, pl, used, px_ok, need_both, min_sin2, max_res, X, rs + 2, early);
                bits = (second ? 2 : 1) | (used << 2);
            } else {
                const double x2 = a2[2 * j], y2 = a2[2 * j + 1];
                double e[3], M[9], b[3], X0[3];
                tri_ray(cam2, x2, y2, e);
#pragma unroll
                for (int a = 0; a < 9; a++) M[a] = 0;
                b[0] = b[1] = b[2] = 0;
                fused_add_ray(1.0, d, cam1.o, M, b);
                fused_add_ray(1.0, e, cam2.o, M, b);
                acc = px_ok && isfinite(x2) && isfinite(y2) && gauss_solve<3>(M, b, X0);
                const double s1 = ((X0[0] - cam1.o[0]) * d[0] + (X0[1] - cam1.o[1]) * d[1]) + (X0[2] - cam1.o[2]) * d[2];
                const double s2 = ((X0[0] - cam2.o[0]) * e[0] + (X0[1] - cam2.o[1]) * e[1]) + (X0[2] - cam2.o[2]) * e[2];
                acc = acc && s1 > 0 && s2 > 0 && isfinite(s1) && isfinite(s2);
                const double w1 = cam1.k0 / (s1 * sigma_px), w2 = cam2.k0 / (s2 * sigma_px);
#pragma unroll
                for (int a = 0; a < 9; a++) M[a] = 0;
                b[0] = b[1] = b[2] = 0;
                fused_add_ray(w1 * w1, d, cam1.o, M, b);
                fused_add_ray(w2 * w2, e, cam2.o, M, b);
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    if (!(used & (1 << c))) continue;
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int q = 0; q < 3; q++) M[3 * r + q] = M[3 * r + q] + wp2 * (pl[c][r] * pl[c][q]);
                        b[r] = b[r] - wp2 * (pl[c][3] * pl[c][r]);
                    }
                }
                acc = gauss_solve<3>(M, b, X) && acc && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
                rs[0] = fused_ray_res(X, cam1.o, d, cam1.k0);
                rs[1] = fused_ray_res(X, cam2.o, e, cam2.k0);
#pragma unroll
                for (int c = 0; c < 2; c++)
                    if (used & (1 << c)) rs[2 + c] = ((pl[c][0] * X[0] + pl[c][1] * X[1]) + pl[c][2] * X[2]) + pl[c][3];
                acc = acc && isfinite(rs[0]) && isfinite(rs[1]) && rs[0] >= 0 && rs[1] >= 0 && isfinite(rs[2]) && isfinite(rs[3]);
                if (max_px > 0 && (rs[0] > max_px || rs[1] > max_px)) acc = false;
                if (max_res > 0 && (fabs(rs[2]) > max_res || fabs(rs[3]) > max_res)) acc = false;
                bits = 3 | (used << 2);
            }
        }
        const unsigned long long bal = __ballot(acc);
        n_ref += __popcll(__ballot(cand && !acc));
        const int slot = m + __popcll(bal & below);
        const bool wr = acc && slot < MAXP;                                        // the table is full: the rest is counted and dropped
        n_trunc += __popcll(__ballot(acc && !wr));
        n_pair += __popcll(__ballot(wr && j >= 0));
        n_left += __popcll(__ballot(wr && j < 0 && !second));
        n_right += __popcll(__ballot(wr && second));
        if (wr) {
            const size_t o = base + (size_t)slot;
            o_X[o * 3] = X[0]; o_X[o * 3 + 1] = X[1]; o_X[o * 3 + 2] = X[2];
            o_idx[o * 2] = v[0]; o_idx[o * 2 + 1] = v[1];
            o_res[o * 4] = rs[0]; o_res[o * 4 + 1] = rs[1]; o_res[o * 4 + 2] = rs[2]; o_res[o * 4 + 3] = rs[3];
            o_src[o * 3] = bits; o_src[o * 3 + 1] = second ? j : k; o_src[o * 3 + 2] = second ? k : j;
            ray2 = ray2 + (rs[0] * rs[0] + rs[1] * rs[1]);
            raymax = fmax(raymax, fmax(rs[0], rs[1]));
            pl2 = pl2 + (rs[2] * rs[2] + rs[3] * rs[3]);
            plmax = fmax(plmax, fmax(fabs(rs[2]), fabs(rs[3])));
        }
        n_rays += 2 * __popcll(__ballot(wr && j >= 0));
        n_planes += __popcll(__ballot(wr && (used & 1))) + __popcll(__ballot(wr && (used & 2)));
        m = min(m + __popcll(bal), MAXP);
    }
    ray2 = wave_sum(ray2);
    pl2 = wave_sum(pl2);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        raymax = fmax(raymax, __shfl_xor(raymax, off, 64));
        plmax = fmax(plmax, __shfl_xor(plmax, off, 64));
    }
    if (lane == 0) {
        o_m[f] = m;
        o_counts[6 * f] = m; o_counts[6 * f + 1] = n_pair; o_counts[6 * f + 2] = n_left; o_counts[6 * f + 3] = n_right;
        o_counts[6 * f + 4] = n_ref; o_counts[6 * f + 5] = n_trunc;
        o_stats[4 * f] = n_rays > 0 ? sqrt(ray2 / (double)n_rays) : 0.0;
        o_stats[4 * f + 1] = n_rays > 0 ? raymax : 0.0;
        o_stats[4 * f + 2] = n_planes > 0 ? sqrt(pl2 / (double)n_planes) : 0.0;
        o_stats[4 * f + 3] = n_planes > 0 ? plmax : 0.0;
        o_flags[f] = n_trunc > 0 ? CPE_FUSED_FLAG_TRUNCATED : 0;
    }
}
// ------------------------------------------------------------------------------------------ projector model
// BUILD-DEFINED (include/cpe.h cpe_fit_projector_model, whose numbered rule this follows): the two pencils of laser planes
// n = a_k + v b_k through one centre C, fitted to the points of many frames through the moments of every line.
//   x = C[3], a_0[3], b_0[3], a_1[3], b_1[3]; a step has 13 numbers: dC, then per family two tangent coordinates of a_k and db_k.
//   info[6] is the "a mask byte changed" flag of the running round and info[7] the "loop has ended" flag; both are 0 on return.
constexpr int PM_NX = 15, PM_NP = 13, PM_MOM = 12;

// unit normal nh of line v of family fam under x, C - relative quantities left to the caller -> |a + v b|
__device__ __forceinline__ double pm_normal(const double *x, int fam, int v, double *nh)
{
    const double *a = x + 3 + 6 * fam, *b = a + 3;
    const double dv = (double)v;
    const double n0 = a[0] + dv * b[0], n1 = a[1] + dv * b[1], n2 = a[2] + dv * b[2];
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    nh[0] = n0 / len; nh[1] = n1 / len; nh[2] = n2 / len;
    return len;
}

// an orthonormal basis e1, e2 of the tangent plane of the unit sphere at a: the coordinate axis of the smallest |a_i| (the first
// of them) with its part along a removed, and a x e1
__device__ __forceinline__ void pm_tangent(const double *a, double *e1, double *e2)
{
    const double a0 = fabs(a[0]), a1 = fabs(a[1]), a2 = fabs(a[2]);
    double ax[3] = {0, 0, 0};
    if (a0 <= a1 && a0 <= a2) ax[0] = 1; else if (a1 <= a2) ax[1] = 1; else ax[2] = 1;
    const double d = (ax[0] * a[0] + ax[1] * a[1]) + ax[2] * a[2];
    double t[3] = {ax[0] - d * a[0], ax[1] - d * a[1], ax[2] - d * a[2]};
    const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    e1[0] = t[0] / tn; e1[1] = t[1] / tn; e1[2] = t[2] / tn;
    cross3(a, e1, e2);
}

// position of (a, b), a <= b, in the upper triangle of an N x N matrix packed by rows
template <int N>
__device__ __forceinline__ constexpr int tri_at(int a, int b) { return a * N - a * (a - 1) / 2 + (b - a); }

// The model as lm_minimize takes it, everything from the moments of the lines: with y = X - C of a kept point of line (k, v),
// n = a_k + v b_k, nh = n / |n|, Q = (I - nh nh') / |n|:  r = nh.y,  dr/dC = -nh,  dr/dt = E' Q y (E = e1 e2 of pm_tangent),
// dr/db = v Q y.  Over the line, sum 1 = N, sum y = s = N (m - C), sum y y' = M = S + N (m - C)(m - C)', so with D = [E' Q; v Q]
// (5 x 3):  J'J = [N nh nh', -nh (D s)'; ., D M D'],  J'r = [-nh (nh.s); D M nh],  sum r^2 = nh' M nh.
// Lane l takes the lines l, l + 64, ... of a family; the 64-lane tree; family 0 before family 1.
struct PmProblem {
    const double *mom;
    int L, lo, lane;
    __device__ __forceinline__ double operator()(const double *x) const
    {
        double acc = 0.0;
        for (int i = lane; i < 2 * L; i += 64) {
            const double *q = mom + PM_MOM * i;
            if (!(q[0] > 0)) continue;
            const int fam = i >= L ? 1 : 0;
            double nh[3];
            pm_normal(x, fam, lo + (i - fam * L), nh);
            const double d0 = q[1] - x[0], d1 = q[2] - x[1], d2 = q[3] - x[2];
            const double nd = (nh[0] * d0 + nh[1] * d1) + nh[2] * d2;
            const double t0 = (q[4] * nh[0] + q[5] * nh[1]) + q[6] * nh[2], t1 = (q[5] * nh[0] + q[7] * nh[1]) + q[8] * nh[2],
                         t2 = (q[6] * nh[0] + q[8] * nh[1]) + q[9] * nh[2];
            acc = acc + (((nh[0] * t0 + nh[1] * t1) + nh[2] * t2) + q[0] * nd * nd);
        }
        return wave_sum(acc);
    }
    __device__ __forceinline__ void normal(const double *x, double *A, double *g) const
    {
#pragma unroll
        for (int k = 0; k < PM_NP * (PM_NP + 1) / 2; k++) A[k] = 0.0;
#pragma unroll
        for (int k = 0; k < PM_NP; k++) g[k] = 0.0;
#pragma unroll
        for (int fam = 0; fam < 2; fam++) {
            double acc[44];   // the 8 x 8 of (C, t, b) of this family, upper triangle by rows, then its J'r
#pragma unroll
            for (int k = 0; k < 44; k++) acc[k] = 0.0;
            double e1[3], e2[3];
            pm_tangent(x + 3 + 6 * fam, e1, e2);
            for (int i = lane; i < L; i += 64) {
                const double *q = mom + PM_MOM * (fam * L + i);
                const double N = q[0];
                if (!(N > 0)) continue;
                const double dv = (double)(lo + i);
                double nh[3];
                const double len = pm_normal(x, fam, lo + i, nh);
                const double d[3] = {q[1] - x[0], q[2] - x[1], q[3] - x[2]};
                const double s[3] = {N * d[0], N * d[1], N * d[2]};
                const double M[9] = {q[4] + s[0] * d[0], q[5] + s[0] * d[1], q[6] + s[0] * d[2],
                                     q[5] + s[0] * d[1], q[7] + s[1] * d[1], q[8] + s[1] * d[2],
                                     q[6] + s[0] * d[2], q[8] + s[1] * d[2], q[9] + s[2] * d[2]};
                double Q[9], D[15];
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b = 0; b < 3; b++) Q[a * 3 + b] = ((a == b ? 1.0 : 0.0) - nh[a] * nh[b]) / len;
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    D[b] = (e1[0] * Q[b] + e1[1] * Q[3 + b]) + e1[2] * Q[6 + b];
                    D[3 + b] = (e2[0] * Q[b] + e2[1] * Q[3 + b]) + e2[2] * Q[6 + b];
#pragma unroll
                    for (int a = 0; a < 3; a++) D[(2 + a) * 3 + b] = dv * Q[a * 3 + b];
                }
                double DM[15], Ds[5], gp[5];
#pragma unroll
                for (int a = 0; a < 5; a++) {
#pragma unroll
                    for (int b = 0; b < 3; b++) DM[a * 3 + b] = (D[a * 3] * M[b] + D[a * 3 + 1] * M[3 + b]) + D[a * 3 + 2] * M[6 + b];
                    Ds[a] = (D[a * 3] * s[0] + D[a * 3 + 1] * s[1]) + D[a * 3 + 2] * s[2];
                    gp[a] = (DM[a * 3] * nh[0] + DM[a * 3 + 1] * nh[1]) + DM[a * 3 + 2] * nh[2];
                }
                const double ns = (nh[0] * s[0] + nh[1] * s[1]) + nh[2] * s[2];
#pragma unroll
                for (int a = 0; a < 3; a++) {
#pragma unroll
                    for (int b = a; b < 3; b++) acc[tri_at<8>(a, b)] = acc[tri_at<8>(a, b)] + N * nh[a] * nh[b];
#pragma unroll
                    for (int b = 0; b < 5; b++) acc[tri_at<8>(a, 3 + b)] = acc[tri_at<8>(a, 3 + b)] - nh[a] * Ds[b];
                    acc[36 + a] = acc[36 + a] - nh[a] * ns;
                }
#pragma unroll
                for (int a = 0; a < 5; a++) {
#pragma unroll
                    for (int b = a; b < 5; b++)
                        acc[tri_at<8>(3 + a, 3 + b)] = acc[tri_at<8>(3 + a, 3 + b)] +
                                                       ((DM[a * 3] * D[b * 3] + DM[a * 3 + 1] * D[b * 3 + 1]) + DM[a * 3 + 2] * D[b * 3 + 2]);
                    acc[36 + 3 + a] = acc[36 + 3 + a] + gp[a];
                }
            }
#pragma unroll
            for (int a = 0; a < 8; a++) {
                const int ga = a < 3 ? a : 3 + 5 * fam + (a - 3);
#pragma unroll
                for (int b = a; b < 8; b++) {
                    const int gb = b < 3 ? b : 3 + 5 * fam + (b - 3);
                    A[tri_at<PM_NP>(ga, gb)] = A[tri_at<PM_NP>(ga, gb)] + wave_sum(acc[tri_at<8>(a, b)]);
                }
                g[ga] = g[ga] + wave_sum(acc[36 + a]);
            }
        }
    }
    // C and b move by their steps; a_k moves in its tangent plane and is brought back to the unit sphere
    __device__ __forceinline__ bool candidate(const double *x, const double *dl, double *xn) const
    {
#pragma unroll
        for (int c = 0; c < 3; c++) xn[c] = x[c] + dl[c];
#pragma unroll
        for (int fam = 0; fam < 2; fam++) {
            const double *a = x + 3 + 6 * fam, *st = dl + 3 + 5 * fam;
            double e1[3], e2[3], t[3];
            pm_tangent(a, e1, e2);
#pragma unroll
            for (int c = 0; c < 3; c++) t[c] = (a[c] + st[0] * e1[c]) + st[1] * e2[c];
            const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                xn[3 + 6 * fam + c] = t[c] / tn;
                xn[6 + 6 * fam + c] = a[3 + c] + st[2 + c];
            }
        }
        return true;
    }
};

// The moments of line (family, index) = blockIdx.x under the mask of this round: the walk of k_index_planes.  Round 0 keeps
// every usable point; a later round keeps the usable points with |nh.(X - C)| < tau under the model of the round before, and
// raises info[6] when a byte of the mask differs from what that round left.  Slot k of the mask is written and read by lane
// k % 64 of this wavefront only.
__global__ __launch_bounds__(64) void k_pm_moments(const double *__restrict__ X, const int *__restrict__ idx, const int *__restrict__ cnt,
                                                   int n, const uint8_t *__restrict__ use, const int *__restrict__ frame_ok, int lo, int L,
                                                   int round, double tau, const double *__restrict__ model, int *info,
                                                   double *__restrict__ o_mom, int *__restrict__ o_count, int *__restrict__ o_frames,
                                                   uint8_t *o_mask)
{
    if (round > 0 && info[7] != 0) return;
    const int line = blockIdx.x, lane = threadIdx.x;   // line = family * L + (v - lo)
    const int fam = line / L, v = lo + (line - fam * L);
    uint8_t *mk = o_mask + (size_t)fam * (size_t)n * MAXP;
    double nh[3] = {0, 0, 0}, Cc[3] = {0, 0, 0};
    if (round > 0) {
        double x[PM_NX];
#pragma unroll
        for (int k = 0; k < PM_NX; k++) x[k] = model[k];
        pm_normal(x, fam, v, nh);
        Cc[0] = x[0]; Cc[1] = x[1]; Cc[2] = x[2];
    }
    int frames = 0, changed = 0;
    bool first = true;
    auto each = [&](auto body) {
        for (int f = 0; f < n; f++) {
            if (frame_ok && frame_ok[f] == 0) continue;
            const int c = min(max(cnt[f], 0), MAXP);
            const size_t base = (size_t)f * MAXP;
            bool any = false;
            for (int k = lane; k < c; k += 64) {
                if (idx[(base + k) * 2 + fam] != v) continue;
                if (use && use[base + k] == 0) continue;
                const double *p = X + (base + k) * 3;
                if (!finite3(p)) continue;
                if (first) {
                    uint8_t in = 1;
                    if (round > 0) {
                        const double r = (nh[0] * (p[0] - Cc[0]) + nh[1] * (p[1] - Cc[1])) + nh[2] * (p[2] - Cc[2]);
                        in = fabs(r) < tau ? 1 : 0;
                        changed |= in != mk[base + k];
                    }
                    mk[base + k] = in;
                    if (!in) continue;
                } else if (!mk[base + k]) continue;
                body(p);
                any = true;
            }
            if (first && __ballot(any) != 0ull) frames++;
        }
        first = false;
    };
    int N;
    double c[3], q[6];
    plane_sums(each, N, c, q);
    if (round > 0 && __ballot(changed) != 0ull && lane == 0) atomicOr(&info[6], 1);
    if (lane == 0) {
        double *o = o_mom + (size_t)line * PM_MOM;
        o[0] = (double)N;
        o[1] = N > 0 ? c[0] : 0.0; o[2] = N > 0 ? c[1] : 0.0; o[3] = N > 0 ? c[2] : 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) o[4 + a] = q[a];
        o[10] = 0; o[11] = 0;
        o_count[line] = N; o_frames[line] = frames;
    }
}

// One wavefront: the model from the moments.  Round 0 starts in closed form (or from x0_in), a later round from the model of
// the round before; see the header for the start and the failures.
__global__ __launch_bounds__(64) void k_pm_solve(const double *__restrict__ mom, const int *__restrict__ frames, int lo, int L, int round,
                                                 double min_spread, double tolx, double tolf, int maxiter,
                                                 const double *__restrict__ x0_in, double *model, int *info)
{
    __shared__ double sN[2 * CPE_MAXL * 3];   // the free plane's normal of every line
    __shared__ int sUse[2 * CPE_MAXL];
    const int lane = threadIdx.x;
    if (round > 0) {
        if (info[7] != 0) return;                                     // the loop has ended
        if (info[6] == 0) { if (lane == 0) info[7] = 1; return; }     // no byte of the mask changed: the model stands
    }
    const int it_before = round > 0 ? info[2] : 0, ev_before = round > 0 ? info[3] : 0;
    // free planes
    int kept0 = 0, kept1 = 0, use0 = 0, use1 = 0;
    for (int i = lane; i < 2 * L; i += 64) {
        const double *q = mom + PM_MOM * i;
        const int N = (int)q[0];
        if (i < L) kept0 += N; else kept1 += N;
        const double Cv[9] = {q[4], q[5], q[6], q[5], q[7], q[8], q[6], q[8], q[9]};
        double w[3], V[9];
        eig3(Cv, w, V);
        bool ok = N >= 3 && frames[i] >= 2 && w[2] > 0;
        ok = ok && !(w[1] / w[2] < min_spread) && isfinite(V[0]) && isfinite(V[3]) && isfinite(V[6]);
        sUse[i] = ok ? 1 : 0;
        sN[3 * i] = V[0]; sN[3 * i + 1] = V[3]; sN[3 * i + 2] = V[6];
        if (ok) { if (i < L) use0++; else use1++; }
    }
    kept0 = wave_sum_i(kept0); kept1 = wave_sum_i(kept1); use0 = wave_sum_i(use0); use1 = wave_sum_i(use1);
    __syncthreads();
    auto fail = [&]() {
        if (lane < 16) model[lane] = 0;
        if (lane == 0) {
            info[0] = CPE_ST_FEW_POINTS; info[1] = round; info[2] = it_before; info[3] = ev_before; info[4] = kept0; info[5] = kept1;
            info[6] = 0; info[7] = 1;
        }
    };
    if (use0 < 2 || use1 < 2) { fail(); return; }
    double x0[PM_NX];
    if (round > 0) {
#pragma unroll
        for (int k = 0; k < PM_NX; k++) x0[k] = model[k];
    } else if (x0_in != nullptr) {
#pragma unroll
        for (int k = 0; k < PM_NX; k++) x0[k] = x0_in[k];
    } else {
        // C: the point nearest to the free planes, (sum n n') C = sum n (n.m)
        double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = lane; i < 2 * L; i += 64) {
            if (!sUse[i]) continue;
            const double *q = mom + PM_MOM * i;
            const double j[3] = {sN[3 * i], sN[3 * i + 1], sN[3 * i + 2]};
            normal_accumulate<3>(j, (j[0] * q[1] + j[1] * q[2]) + j[2] * q[3], acc);
        }
#pragma unroll
        for (int a = 0; a < 9; a++) acc[a] = wave_sum(acc[a]);
        double M[9] = {acc[0], acc[1], acc[2], acc[1], acc[3], acc[4], acc[2], acc[4], acc[5]};
        double rhs[3] = {acc[6], acc[7], acc[8]};
        if (!gauss_solve<3>(M, rhs, x0) || !finite3(x0)) { fail(); return; }
        bool good = true;
#pragma unroll
        for (int fam = 0; fam < 2; fam++) {
            // u: the axis of the pencil, the direction every normal is perpendicular to
            double sc[6] = {0, 0, 0, 0, 0, 0}, sv = 0;
            long long key = LLONG_MAX;
            for (int i = lane; i < L; i += 64) {
                if (!sUse[fam * L + i]) continue;
                const double *nn = sN + 3 * (fam * L + i);
                sc[0] = sc[0] + nn[0] * nn[0]; sc[1] = sc[1] + nn[0] * nn[1]; sc[2] = sc[2] + nn[0] * nn[2];
                sc[3] = sc[3] + nn[1] * nn[1]; sc[4] = sc[4] + nn[1] * nn[2]; sc[5] = sc[5] + nn[2] * nn[2];
                const long long v = (long long)lo + i;
                sv = sv + (double)v;
                const long long kk = (v < 0 ? -v : v) * 512 + i;     // nearest to v = 0, the lower index on a tie
                if (kk < key) key = kk;
            }
#pragma unroll
            for (int a = 0; a < 6; a++) sc[a] = wave_sum(sc[a]);
            sv = wave_sum(sv);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { const long long o = __shfl_xor(key, off, 64); if (o < key) key = o; }
            const double Cv[9] = {sc[0], sc[1], sc[2], sc[1], sc[3], sc[4], sc[2], sc[4], sc[5]};
            double w[3], V[9];
            eig3(Cv, w, V);
            const double u[3] = {V[0], V[3], V[6]};
            const int iref = (int)(key % 512);
            double e1[3] = {sN[3 * (fam * L + iref)], sN[3 * (fam * L + iref) + 1], sN[3 * (fam * L + iref) + 2]}, e2[3];
            {
                const double a0 = fabs(e1[0]), a1 = fabs(e1[1]), a2 = fabs(e1[2]);
                const double big = (a0 >= a1 && a0 >= a2) ? e1[0] : (a1 >= a2 ? e1[1] : e1[2]);
                if (big < 0) { e1[0] = -e1[0]; e1[1] = -e1[1]; e1[2] = -e1[2]; }
                const double du = (e1[0] * u[0] + e1[1] * u[1]) + e1[2] * u[2];
#pragma unroll
                for (int c = 0; c < 3; c++) e1[c] = e1[c] - du * u[c];
                const double en = sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]);
#pragma unroll
                for (int c = 0; c < 3; c++) e1[c] = e1[c] / en;
                cross3(u, e1, e2);
            }
            // tan(theta_v) ~ alpha + beta v over the usable lines, v centred
            const double nu = (double)(fam == 0 ? use0 : use1), vbar = sv / nu;
            double st = 0, svv = 0, svt = 0;
            for (int i = lane; i < L; i += 64) {
                if (!sUse[fam * L + i]) continue;
                const double *nn = sN + 3 * (fam * L + i);
                const double t = ((nn[0] * e2[0] + nn[1] * e2[1]) + nn[2] * e2[2]) / ((nn[0] * e1[0] + nn[1] * e1[1]) + nn[2] * e1[2]);
                const double dv = (double)((long long)lo + i) - vbar;
                st = st + t; svv = svv + dv * dv; svt = svt + dv * t;
            }
            st = wave_sum(st); svv = wave_sum(svv); svt = wave_sum(svt);
            const double beta = svt / svv, alpha = st / nu - beta * vbar;
            double a[3] = {e1[0] + alpha * e2[0], e1[1] + alpha * e2[1], e1[2] + alpha * e2[2]};
            const double an = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                x0[3 + 6 * fam + c] = a[c] / an;
                x0[6 + 6 * fam + c] = beta * e2[c] / an;
            }
            good = good && svv > 0;
        }
        if (!good) { fail(); return; }
    }
    PmProblem prob{mom, L, lo, lane};
    const double f0 = prob(x0);
    bool fin = isfinite(f0);
#pragma unroll
    for (int k = 0; k < PM_NX; k++) fin = fin && isfinite(x0[k]);
    if (!fin) { fail(); return; }
    double x[PM_NX], fx;
    int itercount, func_evals = 1;
    lm_minimize<PM_NP, PM_NX>(prob, x0, f0, tolx, tolf, maxiter, x, fx, itercount, func_evals);
    {
        // The LM accepts a trial only when the objective falls, so it cannot place x better than the rounding of the objective
        // lets it see: sqrt(eps f / curvature), 4e-8 mm along the weakest direction of C on 12 boards and 8e-7 mm where a
        // mis-numbered frame leaves f = 4000.  Closing Gauss-Newton steps of the undamped system go below that: at most 10, each
        // taken when it does not raise the objective beyond its rounding, until one is no longer than tolx.
#pragma nounroll
        for (int closing = 0; closing < 10; closing++) {
            double A[PM_NP * (PM_NP + 1) / 2], g[PM_NP], dl[PM_NP], xn[PM_NX];
            prob.normal(x, A, g);
            if (!lm_damped_solve<PM_NP>(A, g, 0.0, dl) || !prob.candidate(x, dl, xn)) break;
            const double fn = prob(xn);
            func_evals++;
            bool take = fn <= fx + 1e-12 * (1.0 + fx);
            double dmax = 0;
#pragma unroll
            for (int k = 0; k < PM_NP; k++) dmax = fmax(dmax, fabs(dl[k]));
#pragma unroll
            for (int k = 0; k < PM_NX; k++) take = take && isfinite(xn[k]);
            if (!take) break;
#pragma unroll
            for (int k = 0; k < PM_NX; k++) x[k] = xn[k];
            fx = fn;
            if (dmax <= tolx) break;
        }
    }
    fin = isfinite(fx);
#pragma unroll
    for (int k = 0; k < PM_NX; k++) fin = fin && isfinite(x[k]);
    if (!fin) { fail(); return; }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < PM_NX; k++) model[k] = x[k];
        model[15] = fx;
        info[0] = CPE_ST_OK; info[1] = round; info[2] = it_before + itercount; info[3] = ev_before + func_evals;
        info[4] = kept0; info[5] = kept1; info[6] = 0;
        if (round == 0) info[7] = 0;
    }
}

// Blocks 0..n-1: frame_counts of frame blockIdx.x = residuals used and trimmed, per family.  Block n: every line's rms under the
// final model into its moments, and the loop's two flags back to 0.
__global__ __launch_bounds__(64) void k_pm_finish(const double *__restrict__ X, const int *__restrict__ idx, const int *__restrict__ cnt,
                                                  int n, const uint8_t *__restrict__ use, const int *__restrict__ frame_ok, int lo, int L,
                                                  const double *__restrict__ model, int *info, double *o_mom,
                                                  const uint8_t *__restrict__ mask, int *__restrict__ o_fc)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f == n) {
        const bool ok = info[0] == CPE_ST_OK;
        double x[PM_NX];
#pragma unroll
        for (int k = 0; k < PM_NX; k++) x[k] = model[k];
        for (int i = lane; i < 2 * L; i += 64) {
            double *q = o_mom + PM_MOM * (size_t)i;
            double rms = 0.0;
            if (ok && q[0] > 0) {
                const int fam = i >= L ? 1 : 0;
                double nh[3];
                pm_normal(x, fam, lo + (i - fam * L), nh);
                const double d0 = q[1] - x[0], d1 = q[2] - x[1], d2 = q[3] - x[2];
                const double nd = (nh[0] * d0 + nh[1] * d1) + nh[2] * d2;
                const double t0 = (q[4] * nh[0] + q[5] * nh[1]) + q[6] * nh[2], t1 = (q[5] * nh[0] + q[7] * nh[1]) + q[8] * nh[2],
                             t2 = (q[6] * nh[0] + q[8] * nh[1]) + q[9] * nh[2];
                rms = sqrt(fmax((((nh[0] * t0 + nh[1] * t1) + nh[2] * t2) + q[0] * nd * nd) / q[0], 0.0));
            }
            q[10] = rms;
        }
        if (lane == 0) { info[6] = 0; info[7] = 0; }
        return;
    }
    int used0 = 0, used1 = 0, trim0 = 0, trim1 = 0;
    if (!(frame_ok && frame_ok[f] == 0)) {
        const int c = min(max(cnt[f], 0), MAXP);
        const size_t base = (size_t)f * MAXP;
        for (int k = lane; k < c; k += 64) {
            if (use && use[base + k] == 0) continue;
            if (!finite3(X + (base + k) * 3)) continue;
            const int v0 = idx[(base + k) * 2], v1 = idx[(base + k) * 2 + 1];
            if (v0 >= lo && v0 - lo < L) { if (mask[base + k]) used0++; else trim0++; }
            if (v1 >= lo && v1 - lo < L) { if (mask[(size_t)n * MAXP + base + k]) used1++; else trim1++; }
        }
    }
    used0 = wave_sum_i(used0); trim0 = wave_sum_i(trim0); used1 = wave_sum_i(used1); trim1 = wave_sum_i(trim1);
    if (lane == 0) { o_fc[4 * f] = used0; o_fc[4 * f + 1] = trim0; o_fc[4 * f + 2] = used1; o_fc[4 * f + 3] = trim1; }
}

// the table of a model for the indices lo..hi: one lane per line, lines in rounds of 64
__global__ __launch_bounds__(64) void k_pm_table(const double *__restrict__ model, const int *__restrict__ info, int lo, int L,
                                                 double *__restrict__ o_P, int *__restrict__ o_status, double *__restrict__ o_centre,
                                                 int *__restrict__ o_cstatus)
{
    const int lane = threadIdx.x;
    const bool ok = info[0] == CPE_ST_OK;
    double x[PM_NX];
#pragma unroll
    for (int k = 0; k < PM_NX; k++) x[k] = model[k];
    for (int i = lane; i < 2 * L; i += 64) {
        const int fam = i >= L ? 1 : 0;
        double nh[3];
        const double len = pm_normal(x, fam, (int)((long long)lo + (i - fam * L)), nh);
        const bool lok = ok && len > 0 && finite3(nh);
        const double a0 = fabs(nh[0]), a1 = fabs(nh[1]), a2 = fabs(nh[2]);
        const double big = (a0 >= a1 && a0 >= a2) ? nh[0] : (a1 >= a2 ? nh[1] : nh[2]);
        if (big < 0) { nh[0] = -nh[0]; nh[1] = -nh[1]; nh[2] = -nh[2]; }
        double *P = o_P + 4 * (size_t)i;
        P[0] = lok ? nh[0] : 0.0; P[1] = lok ? nh[1] : 0.0; P[2] = lok ? nh[2] : 0.0;
        P[3] = lok ? -((nh[0] * x[0] + nh[1] * x[1]) + nh[2] * x[2]) : 0.0;
        o_status[i] = lok ? CPE_ST_OK : CPE_ST_FEW_POINTS;
    }
    if (lane == 0) {
        const int kept = info[4] + info[5];
        o_centre[0] = ok ? x[0] : 0.0; o_centre[1] = ok ? x[1] : 0.0; o_centre[2] = ok ? x[2] : 0.0;
        o_centre[3] = ok && kept > 0 ? sqrt(fmax(model[15], 0.0) / (double)kept) : 0.0;
        o_cstatus[0] = ok ? CPE_ST_OK : CPE_ST_FEW_POINTS;
    }
}

// ------------------------------------------------------------------------------------------ index shift of stereo frames
// BUILD-DEFINED (include/cpe.h cpe_index_shift_batch, whose numbered rule this follows): a stereo point's position does not
// depend on its index, so the points of a frame and a table that is right for most frames give the frame's shift: per index
// component, the d for which the most points lie on the plane of index + d.  One wavefront per (frame, component), lane l takes
// points l, l + 64, ...  The component's family of the table (at most 256 planes and statuses, 9 KB) is copied to LDS first:
// a point reads up to 17 neighbouring planes, so a frame of 250 points reads 8 times the table.  The candidate counters are a
// register array behind loops unrolled over the compile-time 17 candidates and predicated on |d| <= win.
constexpr int SHIFT_W = CPE_SHIFT_MAX_WIN, SHIFT_NC = 2 * CPE_SHIFT_MAX_WIN + 1;

__global__ __launch_bounds__(64) void k_index_shift(const double *__restrict__ X, const int *__restrict__ idx, const int *__restrict__ cnt,
                                                    const uint8_t *__restrict__ use, const double *__restrict__ P,
                                                    const int *__restrict__ line_status, int lo, int hi, int win0, int win1, double tau,
                                                    int min_score, int swap, int *__restrict__ o_shift, int *__restrict__ o_score,
                                                    int *__restrict__ o_scores, double *__restrict__ o_rms, int *__restrict__ o_flags,
                                                    int *__restrict__ o_idx)
{
    __shared__ double sP[CPE_MAXL * 4];
    __shared__ int sS[CPE_MAXL];
    const int f = blockIdx.x >> 1, c = blockIdx.x & 1, lane = threadIdx.x;
    const int n = min(max(cnt[f], 0), MAXP);
    const int L = hi - lo + 1;                     // 1..CPE_MAXL, checked by the host
    const int win = c ? win1 : win0;               // 0..SHIFT_W, checked by the host
    const size_t base = (size_t)f * MAXP;
    {
        const size_t fam = (size_t)((c ^ swap) * L);
        for (int i = lane; i < 4 * L; i += 64) sP[i] = P[fam * 4 + i];
        for (int i = lane; i < L; i += 64) sS[i] = line_status[fam + i];
    }
    __syncthreads();
    // rel = idx - lo of a point that can count at all lies in [-win, L - 1 + win]: tested in 64 bits, before any addition
    const long long rlo = -(long long)win, rhi = (long long)(L - 1 + win);
    int sc[SHIFT_NC];
#pragma unroll
    for (int j = 0; j < SHIFT_NC; j++) sc[j] = 0;
    int usable = 0;
    for (int k = lane; k < n; k += 64) {
        if (use && use[base + k] == 0) continue;
        if (!finite3(X + (base + k) * 3)) continue;
        usable++;
        const long long rl = (long long)idx[(base + k) * 2 + c] - (long long)lo;
        if (rl < rlo || rl > rhi) continue;
        const int rel = (int)rl;
        const double x = X[(base + k) * 3], y = X[(base + k) * 3 + 1], z = X[(base + k) * 3 + 2];
#pragma unroll
        for (int j = 0; j < SHIFT_NC; j++) {
            const int r = rel + (j - SHIFT_W);
            if (abs(j - SHIFT_W) <= win && r >= 0 && r < L && sS[r] == CPE_ST_OK) {
                const double e = ((sP[4 * r] * x + sP[4 * r + 1] * y) + sP[4 * r + 2] * z) + sP[4 * r + 3];
                if (fabs(e) < tau) sc[j]++;
            }
        }
    }
    usable = wave_sum_i(usable);
#pragma unroll
    for (int j = 0; j < SHIFT_NC; j++) sc[j] = wave_sum_i(sc[j]);
    // winner: the smallest key (-score, |d|, d); then the second-largest value among the candidates
    int best = -1, wd = 0;
#pragma unroll
    for (int j = 0; j < SHIFT_NC; j++) {
        const int d = j - SHIFT_W, a = abs(d);
        if (a <= win && (sc[j] > best || (sc[j] == best && (a < abs(wd) || (a == abs(wd) && d < wd))))) { best = sc[j]; wd = d; }
    }
    int second = 0, at0 = 0, mine = 0;
#pragma unroll
    for (int j = 0; j < SHIFT_NC; j++) {
        const int d = j - SHIFT_W;
        if (abs(d) <= win && d != wd) second = max(second, sc[j]);
        if (d == 0) at0 = sc[j];
        if (lane == j) mine = sc[j];
    }
    int flags = 0, d_app = wd;
    if (!(best >= min_score && best >= 2 * second)) { flags |= CPE_SHIFT_FLAG_WEAK; d_app = 0; }
    if (win > 0 && abs(wd) == win) flags |= CPE_SHIFT_FLAG_EDGE;
    if (d_app != 0) flags |= CPE_SHIFT_FLAG_SHIFTED;
    if (o_scores && lane >= SHIFT_W - win && lane <= SHIFT_W + win)
        o_scores[(size_t)f * (2 * win0 + 1 + 2 * win1 + 1) + (c ? 2 * win0 + 1 : 0) + (lane - (SHIFT_W - win))] = mine;
    // second pass: the counted points' squared residuals at the applied shift and at d = 0; idx + shift on the way
    double sa = 0.0, s0 = 0.0;
    int ca = 0, c0 = 0;
    for (int k = lane; k < n; k += 64) {
        const int v = idx[(base + k) * 2 + c];
        o_idx[(base + k) * 2 + c] = (int)((unsigned)v + (unsigned)d_app);       // (a garbage index wraps, it does not overflow)
        if (use && use[base + k] == 0) continue;
        if (!finite3(X + (base + k) * 3)) continue;
        const long long rl = (long long)v - (long long)lo;
        if (rl < rlo || rl > rhi) continue;
        const double x = X[(base + k) * 3], y = X[(base + k) * 3 + 1], z = X[(base + k) * 3 + 2];
        const int ra = (int)rl + d_app, r0 = (int)rl;
        if (ra >= 0 && ra < L && sS[ra] == CPE_ST_OK) {
            const double e = ((sP[4 * ra] * x + sP[4 * ra + 1] * y) + sP[4 * ra + 2] * z) + sP[4 * ra + 3];
            if (fabs(e) < tau) { sa = sa + e * e; ca++; }
        }
        if (r0 >= 0 && r0 < L && sS[r0] == CPE_ST_OK) {
            const double e = ((sP[4 * r0] * x + sP[4 * r0 + 1] * y) + sP[4 * r0 + 2] * z) + sP[4 * r0 + 3];
            if (fabs(e) < tau) { s0 = s0 + e * e; c0++; }
        }
    }
    sa = wave_sum(sa); s0 = wave_sum(s0); ca = wave_sum_i(ca); c0 = wave_sum_i(c0);
    if (lane == 0) {
        const size_t o = (size_t)f * 2 + c;
        o_shift[o] = d_app;
        o_score[4 * o] = best; o_score[4 * o + 1] = second; o_score[4 * o + 2] = at0; o_score[4 * o + 3] = usable;
        o_rms[2 * o] = ca > 0 ? sqrt(sa / (double)ca) : 0.0;
        o_rms[2 * o + 1] = c0 > 0 ? sqrt(s0 / (double)c0) : 0.0;
        o_flags[o] = flags;
    }
}
}  // namespace

extern "C" int32_t cpe_fit_plane_batch(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n,
                                       const CpePlaneFitParams *params, double *P, double *T, double *grid, double *stats,
                                       int32_t *n_inliers, uint8_t *inlier_mask, int32_t *flags, int32_t *status, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_fit_plane_batch: n < 0");
    CpePlaneFitParams p = {0.0, 4, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.max_rounds >= 0 && p.max_rounds <= CPE_PLANEFIT_MAX_ROUNDS && !(p.tau != p.tau),
                  "cpe_fit_plane_batch: bad CpePlaneFitParams (max_rounds 0..%d, tau not NaN)", CPE_PLANEFIT_MAX_ROUNDS);
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(X && idx && cnt && P && T && grid && stats && n_inliers && inlier_mask && flags && status,
                  "cpe_fit_plane_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_fit_plane, dim3(n), dim3(64), 0, (hipStream_t)stream, X, idx, cnt, p.tau, p.max_rounds, P, T, grid, stats, n_inliers,
                inlier_mask, flags, status);
    CPE_CHECK_LAUNCH("k_fit_plane");
    return CPE_OK;
}

extern "C" int32_t cpe_index_planes_batch(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n, const uint8_t *use,
                                          const int32_t *frame_ok, int32_t lo, int32_t hi, double min_spread, double *P,
                                          double *stats, int32_t *count, int32_t *frames, int32_t *status, double *centre,
                                          int32_t *centre_status, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_index_planes_batch: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_index_planes_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CPE_CHECK_ARG(min_spread >= 0, "cpe_index_planes_batch: min_spread < 0");
    CPE_CHECK_ARG((n == 0 || (X && idx && cnt)) && P && stats && count && frames && status && centre && centre_status,
                  "cpe_index_planes_batch: null pointer");
    const int L = hi - lo + 1;
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_index_planes, dim3(2 * L), dim3(64), 0, (hipStream_t)stream, X, idx, cnt, n, use, frame_ok, lo, L, min_spread, P, stats,
                count, frames, status);
    CPE_CHECK_LAUNCH("k_index_planes");
    CPE_KLAUNCH(k_planes_centre, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)P, (const int *)status, L, centre, centre_status);
    CPE_CHECK_LAUNCH("k_planes_centre");
    return CPE_OK;
}

extern "C" int32_t cpe_table_triangulate_batch(const double *xy, const int32_t *id, const int32_t *cnt, int32_t n, const double *K,
                                               const double *Tc, const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                               const CpeTableTriParams *params, double *X, int32_t *idx, double *res, int32_t *src,
                                               int32_t *m, int32_t *counts, double *stats, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_table_triangulate_batch: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_table_triangulate_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CpeTableTriParams p = {0, 0, 0.01, 0.0};
    if (params) p = *params;
    CPE_CHECK_ARG((p.swap == 0 || p.swap == 1) && (p.need_both == 0 || p.need_both == 1) && p.min_sin >= 0 && !(p.max_res != p.max_res),
                  "cpe_table_triangulate_batch: bad CpeTableTriParams (swap, need_both 0 or 1, min_sin >= 0, max_res not NaN)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(xy && id && cnt && K && P && line_status && X && idx && res && src && m && counts && stats,
                  "cpe_table_triangulate_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_table_triangulate, dim3(n), dim3(64), 0, (hipStream_t)stream, xy, id, cnt, K, Tc, P, line_status, lo, hi, p.swap,
                p.need_both, p.min_sin * p.min_sin, p.max_res, X, idx, res, src, m, counts, stats);
    CPE_CHECK_LAUNCH("k_table_triangulate");
    return CPE_OK;
}

extern "C" int32_t cpe_fused_triangulate_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                               const int32_t *id2, const int32_t *cnt2, int32_t n, const double *K1, const double *K2,
                                               const double *T21, const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                               const CpeFusedTriParams *params, double *X, int32_t *idx, double *res, int32_t *src,
                                               int32_t *m, int32_t *counts, double *stats, int32_t *flags, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_fused_triangulate_batch: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_fused_triangulate_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CpeFusedTriParams p = {0, 0, 0.01, 0.25, 0.02, 0.0, 0.0};
    if (params) p = *params;
    CPE_CHECK_ARG((p.swap == 0 || p.swap == 1) && (p.need_both == 0 || p.need_both == 1) && p.min_sin >= 0 && p.sigma_px > 0 &&
                      p.sigma_px <= DBL_MAX && p.sigma_mm > 0 && p.sigma_mm <= DBL_MAX && !(p.max_res != p.max_res) && !(p.max_px != p.max_px),
                  "cpe_fused_triangulate_batch: bad CpeFusedTriParams (swap, need_both 0 or 1, min_sin >= 0, sigma_px and sigma_mm "
                  "positive and finite, max_res and max_px not NaN)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(xy1 && id1 && cnt1 && xy2 && id2 && cnt2 && K1 && K2 && T21 && P && line_status && X && idx && res && src && m &&
                      counts && stats && flags,
                  "cpe_fused_triangulate_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_fused_triangulate, dim3(n), dim3(64), 0, (hipStream_t)stream, xy1, id1, cnt1, xy2, id2, cnt2, K1, K2, T21, P, line_status,
                lo, hi, p.swap, p.need_both, p.min_sin * p.min_sin, p.sigma_px, p.sigma_mm, p.max_res, p.max_px, X, idx, res, src, m, counts,
                stats, flags);
    CPE_CHECK_LAUNCH("k_fused_triangulate");
    return CPE_OK;
}

extern "C" int32_t cpe_fit_projector_model(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n, const uint8_t *use,
                                           const int32_t *frame_ok, int32_t lo, int32_t hi, const CpeProjectorModelParams *params,
                                           const double *x0, double *model, int32_t *info, double *moments, int32_t *count,
                                           int32_t *frames, uint8_t *inlier_mask, int32_t *frame_counts, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_fit_projector_model: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_fit_projector_model: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CpeProjectorModelParams p = {0.0, 4, 100, 1e-4, 1e-9, 1e-9};
    if (params) p = *params;
    CPE_CHECK_ARG(p.max_rounds >= 0 && p.max_rounds <= CPE_PLANEFIT_MAX_ROUNDS && !(p.tau != p.tau) && p.min_spread >= 0 && p.tolx >= 0 &&
                      p.tolf >= 0 && p.maxiter >= 0,
                  "cpe_fit_projector_model: bad CpeProjectorModelParams (max_rounds 0..%d, tau not NaN, min_spread, tolx, tolf, maxiter >= 0)",
                  CPE_PLANEFIT_MAX_ROUNDS);
    CPE_CHECK_ARG((n == 0 || (X && idx && cnt && inlier_mask && frame_counts)) && model && info && moments && count && frames,
                  "cpe_fit_projector_model: null pointer");
    const int L = hi - lo + 1;
    const int rounds = p.tau > 0 ? p.max_rounds : 0;
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) CPE_CHECK_HIP(hipMemsetAsync(inlier_mask, 0, (size_t)2 * n * CPE_MAXP, s));
    CPE_LAUNCH_BEGIN();
    // every round is enqueued; a round's kernels return at once when the loop has ended (info[7])
    for (int r = 0; r <= rounds; r++) {
        CPE_KLAUNCH(k_pm_moments, dim3(2 * L), dim3(64), 0, s, X, idx, cnt, n, use, frame_ok, lo, L, r, p.tau, (const double *)model, info,
                    moments, count, frames, inlier_mask);
        CPE_CHECK_LAUNCH("k_pm_moments");
        CPE_KLAUNCH(k_pm_solve, dim3(1), dim3(64), 0, s, (const double *)moments, (const int *)frames, lo, L, r, p.min_spread, p.tolx, p.tolf,
                    p.maxiter, x0, model, info);
        CPE_CHECK_LAUNCH("k_pm_solve");
    }
    CPE_KLAUNCH(k_pm_finish, dim3(n + 1), dim3(64), 0, s, X, idx, cnt, n, use, frame_ok, lo, L, (const double *)model, info, moments,
                (const uint8_t *)inlier_mask, frame_counts);
    CPE_CHECK_LAUNCH("k_pm_finish");
    return CPE_OK;
}

extern "C" int32_t cpe_projector_model_table(const double *model, const int32_t *info, int32_t lo, int32_t hi, double *P, int32_t *status,
                                             double *centre, int32_t *centre_status, void *stream)
{
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_projector_model_table: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CPE_CHECK_ARG(model && info && P && status && centre && centre_status, "cpe_projector_model_table: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_pm_table, dim3(1), dim3(64), 0, (hipStream_t)stream, model, info, lo, hi - lo + 1, P, status, centre, centre_status);
    CPE_CHECK_LAUNCH("k_pm_table");
    return CPE_OK;
}

extern "C" int32_t cpe_index_shift_batch(const double *X, const int32_t *idx, const int32_t *cnt, int32_t n, const uint8_t *use,
                                         const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                         const CpeIndexShiftParams *params, int32_t *shift, int32_t *score, int32_t *scores, double *rms,
                                         int32_t *flags, int32_t *idx_out, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_index_shift_batch: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_index_shift_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CpeIndexShiftParams p = {{4, 4}, 1.0, 8, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.win[0] >= 0 && p.win[0] <= CPE_SHIFT_MAX_WIN && p.win[1] >= 0 && p.win[1] <= CPE_SHIFT_MAX_WIN,
                  "cpe_index_shift_batch: window must be 0..%d for both components", CPE_SHIFT_MAX_WIN);
    CPE_CHECK_ARG(p.tau > 0 && p.min_score >= 0 && (p.swap == 0 || p.swap == 1),
                  "cpe_index_shift_batch: bad CpeIndexShiftParams (tau > 0, min_score >= 0, swap 0 or 1)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(X && idx && cnt && P && line_status && shift && score && rms && flags && idx_out, "cpe_index_shift_batch: null pointer");
    CPE_CHECK_ARG(idx_out != idx, "cpe_index_shift_batch: idx_out may not be idx");
    CPE_CHECK_ARG((long long)n * 2 <= INT_MAX, "cpe_index_shift_batch: 2 n exceeds 2^31 - 1");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_index_shift, dim3(2 * n), dim3(64), 0, (hipStream_t)stream, X, idx, cnt, use, P, line_status, lo, hi, p.win[0], p.win[1],
                p.tau, p.min_score, p.swap, shift, score, scores, rms, flags, idx_out);
    CPE_CHECK_LAUNCH("k_index_shift");
    return CPE_OK;
}

// ------------------------------------------------------------------------------------------ re-labelling of the planar tables
// BUILD-DEFINED (include/cpe.h cpe_grid_relabel_batch, whose numbered rule this follows).  One workgroup of two wavefronts per
// image, wavefront c works on id component c in its own half of the LDS (36.3 KB in all) and the two meet at two barriers: after
// the label spans (either may flag the image) and before the points are written (a point needs both its lines).  Reproducible
// bits: the slots of a label are grouped stably -- integer counts per label, a prefix, then the slot lists filled in rounds of
// 64 slots with ranks from ballots -- and one lane per line sums its list from first to last, the reference's order.  Sorting and
// medians of at most 256 lines are ranks by counting; a local median is over at most four values and is taken in registers
// behind a fixed network (no indexed register array: the k_index_shift note on scratch); prefixes run in four rounds of 64 with a
// carried base.
namespace {
constexpr int RL_L = CPE_MAXL;

struct RelabelLds {
    unsigned short list[CPE_MAXP];  // the usable slots grouped by label, in slot order inside a group
    int cnt[RL_L];                  // bin (label - smallest label) -> points
    int cur[RL_L];                  // bin -> where its next slot goes; after the fill: the end of its list
    int slot[RL_L];                 // bin -> line slot (the labels seen, ascending), -1 for an empty bin
    int bin[RL_L];                  // line slot -> bin
    int N[RL_L], state[RL_L], index[RL_L];   // per line slot
    int ord[RL_L];                  // position in the order of rule 4 -> line slot (supported lines)
    int ord2[RL_L];                 // the same of the remaining lines (rule 6)
    int pre[RL_L];                  // remaining line -> the sum of the inc before it
    double p[RL_L];                 // per line slot
    double gap[RL_L];
    double med[2];
};

// LDS operations of one wavefront complete in order; the fence keeps the compiler from moving them across
__device__ __forceinline__ void rl_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// (s[(m-1)/2] + s[m/2]) / 2 of the sorted v[0..m), m >= 1: ranks by counting in (value, position) order
__device__ double rl_median(const double *v, int m, double *med, int lane)
{
    for (int i = lane; i < m; i += 64) {
        const double x = v[i];
        int r = 0;
        for (int j = 0; j < m; j++) {
            const double y = v[j];
            r += (y < x || (y == x && j < i)) ? 1 : 0;
        }
        if (r == (m - 1) / 2) med[0] = x;
        if (r == m / 2) med[1] = x;
    }
    rl_sync();
    const double out = (med[0] + med[1]) / 2.0;
    rl_sync();
    return out;
}

__device__ __forceinline__ void rl_cswap(double &a, double &b)
{
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo; b = hi;
}

__global__ __launch_bounds__(128) void k_grid_relabel(const double *__restrict__ xy, const int *__restrict__ id, const int *__restrict__ cnt,
                                                      const double *__restrict__ center, int swap, int min_pts, double merge_frac, int dir0,
                                                      int dir1, double *__restrict__ o_xy, int *__restrict__ o_id, int *__restrict__ o_cnt,
                                                      int *__restrict__ o_src, int *__restrict__ o_lines, double *__restrict__ o_linep,
                                                      double *__restrict__ o_pitch, int *__restrict__ o_counts, int *__restrict__ o_flags)
{
    __shared__ RelabelLds S[2];
    __shared__ int s_ovf[2], s_few[2], s_lmin[2];
    const int f = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    RelabelLds &W = S[c];
    const int n = min(max(cnt[f], 0), MAXP);
    const size_t base = (size_t)f * MAXP;
    const double cx = center[2 * (size_t)f], cy = center[2 * (size_t)f + 1];
    const int iu = (c ^ swap) == 0 ? 1 : 0, it = 1 - iu;         // which pixel coordinate positions the lines of this component
    const double tc = iu ? cx : cy, uc = iu ? cy : cx;
    const size_t oc = (size_t)f * 2 + c;

    // rules 1, 2: the label span of the usable points
    int lmin = INT_MAX, lmax = INT_MIN;
    for (int k = lane; k < n; k += 64) {
        if (!(isfinite(xy[(base + k) * 2]) && isfinite(xy[(base + k) * 2 + 1]))) continue;
        const int v = id[(base + k) * 2 + c];
        lmin = min(lmin, v); lmax = max(lmax, v);
    }
    lmin = wave_min_i(lmin); lmax = wave_max_i(lmax);
    if (lane == 0) {
        s_ovf[c] = (lmin <= lmax && (long long)lmax - (long long)lmin >= (long long)RL_L) ? 1 : 0;
        s_lmin[c] = lmin;
    }
    __syncthreads();
    const int bad = ((isfinite(cx) && isfinite(cy)) ? 0 : CPE_RELABEL_FLAG_NO_CENTRE) | ((s_ovf[0] | s_ovf[1]) ? CPE_RELABEL_FLAG_OVERFLOW : 0);
    if (bad) {                                                   // (uniform over the workgroup)
        if (lane < 4) o_counts[oc * 4 + lane] = 0;
        if (lane == 0) {
            o_pitch[oc] = 0.0;
            if (c == 0) { o_cnt[f] = 0; o_flags[f] = bad; }
        }
        return;
    }

    // points per label, the lists' starts and the line slots
    for (int i = lane; i < RL_L; i += 64) W.cnt[i] = 0;
    rl_sync();
    for (int k = lane; k < n; k += 64) {
        if (!(isfinite(xy[(base + k) * 2]) && isfinite(xy[(base + k) * 2 + 1]))) continue;
        atomicAdd(&W.cnt[id[(base + k) * 2 + c] - lmin], 1);
    }
    rl_sync();
    int nl = 0;
    {
        int pbase = 0;
        for (int r = 0; r < RL_L / 64; r++) {
            const int b = r * 64 + lane, cn = W.cnt[b];
            int incl = cn;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            W.cur[b] = pbase + incl - cn;
            const unsigned long long bal = __ballot(cn > 0);
            const int sl = nl + __popcll(bal & lt);
            W.slot[b] = cn > 0 ? sl : -1;
            if (cn > 0) W.bin[sl] = b;
            pbase += __shfl(incl, 63, 64);
            nl += __popcll(bal);
        }
    }
    rl_sync();
    // the lists, in rounds of 64 slots: the lanes of one label take their places by their rank among themselves
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        int b = -1;
        if (k < n && isfinite(xy[(base + k) * 2]) && isfinite(xy[(base + k) * 2 + 1])) b = id[(base + k) * 2 + c] - lmin;
        unsigned long long todo = __ballot(b >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lb = __shfl(b, leader, 64);
            const unsigned long long same = __ballot(b == lb);
            if (b == lb) {
                const int at = W.cur[lb];
                W.list[at + __popcll(same & lt)] = (unsigned short)k;
                if (lane == leader) W.cur[lb] = at + __popcll(same);
            }
            rl_sync();
            todo &= ~same;
        }
    }
    rl_sync();

    // rule 3: one lane per line
    for (int ls = lane; ls < nl; ls += 64) {
        const int b = W.bin[ls], N = W.cnt[b], l0 = W.cur[b] - N;
        double st = 0.0, su = 0.0;
        for (int j = 0; j < N; j++) {
            const size_t k = base + W.list[l0 + j];
            st = st + xy[k * 2 + it]; su = su + xy[k * 2 + iu];
        }
        const double tm = st / (double)N, um = su / (double)N;
        double Stt = 0.0, Stu = 0.0;
        for (int j = 0; j < N; j++) {
            const size_t k = base + W.list[l0 + j];
            const double dt = xy[k * 2 + it] - tm, du = xy[k * 2 + iu] - um;
            Stt = Stt + dt * dt; Stu = Stu + dt * du;
        }
        const double a = Stu / Stt, p = um + a * (tc - tm);
        const bool has_p = Stt > 0.0 && isfinite(p);
        W.p[ls] = has_p ? p : 0.0;
        W.N[ls] = N;
        W.state[ls] = (has_p && N >= min_pts) ? CPE_RELABEL_LINE_KEPT : CPE_RELABEL_LINE_UNSUPPORTED;
        W.index[ls] = 0;
    }
    rl_sync();

    // rule 4: the order by (p, label), a line slot being a label's rank; pitch0
    int ns = 0;
    for (int r = 0; r < RL_L / 64; r++) {
        const int ls = r * 64 + lane;
        ns += __popcll(__ballot(ls < nl && W.state[ls] == CPE_RELABEL_LINE_KEPT));
    }
    for (int ls = lane; ls < nl; ls += 64) {
        if (W.state[ls] != CPE_RELABEL_LINE_KEPT) continue;
        const double p = W.p[ls];
        int rk = 0;
        for (int j = 0; j < nl; j++) {
            const double q = W.p[j];
            rk += (W.state[j] == CPE_RELABEL_LINE_KEPT && (q < p || (q == p && j < ls))) ? 1 : 0;
        }
        W.ord[rk] = ls;
    }
    rl_sync();
    for (int i = lane; i < ns - 1; i += 64) W.gap[i] = W.p[W.ord[i + 1]] - W.p[W.ord[i]];
    rl_sync();
    const double pitch0 = ns >= 2 ? rl_median(W.gap, ns - 1, W.med, lane) : 0.0;

    // rule 5: phantoms, all judged on the list of rule 4; the remaining lines are compacted in order
    const double thr = merge_frac * pitch0;
    int nr = 0;
    for (int r = 0; r < RL_L / 64; r++) {
        const int i = r * 64 + lane;
        bool keep = false;
        int ls = 0;
        if (i < ns) {
            ls = W.ord[i];
            const int Ni = W.N[ls];
            bool ph = false;
            if (i > 0 && W.gap[i - 1] < thr && W.N[W.ord[i - 1]] >= Ni) ph = true;
            if (i < ns - 1 && W.gap[i] < thr && W.N[W.ord[i + 1]] > Ni) ph = true;
            keep = !ph;
            if (ph) W.state[ls] = CPE_RELABEL_LINE_PHANTOM;
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) W.ord2[nr + __popcll(bal & lt)] = ls;
        nr += __popcll(bal);
    }
    rl_sync();

    if (nr >= 1) {
        // rule 6: gaps, local pitches, increments and their prefix
        for (int i = lane; i < nr - 1; i += 64) W.gap[i] = W.p[W.ord2[i + 1]] - W.p[W.ord2[i]];
        rl_sync();
        const double med_all = nr >= 2 ? rl_median(W.gap, nr - 1, W.med, lane) : 0.0;
        const int ng = nr - 1;
        int carry = 0;
        for (int r = 0; r < RL_L / 64; r++) {
            const int i = r * 64 + lane;
            int inc = 0;
            if (i < ng) {
                const double g = W.gap[i];
                double v0 = INFINITY, v1 = INFINITY, v2 = INFINITY, v3 = INFINITY;
                int have = 0;
                if (i - 2 >= 0) { v0 = W.gap[i - 2]; have++; }
                if (i - 1 >= 0) { v1 = W.gap[i - 1]; have++; }
                if (i + 1 < ng) { v2 = W.gap[i + 1]; have++; }
                if (i + 2 < ng) { v3 = W.gap[i + 2]; have++; }
                rl_cswap(v0, v1); rl_cswap(v2, v3); rl_cswap(v0, v2); rl_cswap(v1, v3); rl_cswap(v1, v2);   // missing ones go last
                const double pi = have < 2 ? med_all : have == 2 ? (v0 + v1) / 2.0 : have == 3 ? v1 : (v1 + v2) / 2.0;
                inc = 1;
                if (pi > 0.0) {
                    const double q = floor(g / pi + 0.5);
                    if (q >= (double)CPE_RELABEL_MAX_INC) inc = CPE_RELABEL_MAX_INC;
                    else if (q > 1.0) inc = (int)q;
                }
            }
            int incl = inc;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            W.pre[i] = carry + incl - inc;
            carry += __shfl(incl, 63, 64);
        }
        // rule 7: the anchor, the first in order among the nearest
        double bd = INFINITY;
        int bi = INT_MAX;
        for (int i = lane; i < nr; i += 64) {
            const double d = fabs(W.p[W.ord2[i]] - uc);
            if (bi == INT_MAX || d < bd) { bd = d; bi = i; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double od = __shfl_xor(bd, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (oi != INT_MAX && (bi == INT_MAX || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
        }
        rl_sync();
        const int pa = W.pre[bi], dirc = c ? dir1 : dir0;
        for (int i = lane; i < nr; i += 64) W.index[W.ord2[i]] = dirc * (W.pre[i] - pa);
    }
    rl_sync();

    for (int ls = lane; ls < nl; ls += 64) {
        const size_t o = oc * RL_L + ls;
        o_lines[o * 4] = lmin + W.bin[ls]; o_lines[o * 4 + 1] = W.index[ls]; o_lines[o * 4 + 2] = W.N[ls]; o_lines[o * 4 + 3] = W.state[ls];
        o_linep[o] = W.p[ls];
    }
    if (lane == 0) {
        o_counts[oc * 4] = nl; o_counts[oc * 4 + 1] = ns; o_counts[oc * 4 + 2] = ns - nr; o_counts[oc * 4 + 3] = nr;
        o_pitch[oc] = pitch0;
        s_few[c] = nr == 0 ? (CPE_RELABEL_FLAG_FEW_LINES << c) : 0;
    }
    __syncthreads();
    if (c == 1) return;

    // rule 8: wavefront 0 writes the points whose two lines are kept, in slot order
    const int lmin0 = s_lmin[0], lmin1 = s_lmin[1];
    int m = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        bool wr = false;
        double x = 0.0, y = 0.0;
        int i0 = 0, i1 = 0;
        if (k < n) {
            x = xy[(base + k) * 2]; y = xy[(base + k) * 2 + 1];
            if (isfinite(x) && isfinite(y)) {
                const int s0 = S[0].slot[id[(base + k) * 2] - lmin0], s1 = S[1].slot[id[(base + k) * 2 + 1] - lmin1];
                wr = S[0].state[s0] == CPE_RELABEL_LINE_KEPT && S[1].state[s1] == CPE_RELABEL_LINE_KEPT;
                i0 = S[0].index[s0]; i1 = S[1].index[s1];
            }
        }
        const unsigned long long bal = __ballot(wr);
        if (wr) {
            const size_t at = base + m + __popcll(bal & lt);
            o_xy[at * 2] = x; o_xy[at * 2 + 1] = y;
            o_id[at * 2] = i0; o_id[at * 2 + 1] = i1;
            o_src[at] = k;
        }
        m += __popcll(bal);
    }
    if (lane == 0) { o_cnt[f] = m; o_flags[f] = s_few[0] | s_few[1]; }
}

// do two byte ranges share a byte?
bool rl_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}
}  // namespace

extern "C" int32_t cpe_grid_relabel_batch(const double *xy, const int32_t *id, const int32_t *cnt, const double *center, int32_t n,
                                          const CpeRelabelParams *params, double *xy_out, int32_t *id_out, int32_t *cnt_out, int32_t *src,
                                          int32_t *lines, double *line_p, double *pitch, int32_t *counts, int32_t *flags, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_grid_relabel_batch: n < 0");
    CpeRelabelParams p = {0, 3, 0.65, {1, 1}};
    if (params) p = *params;
    CPE_CHECK_ARG(p.min_pts >= 2 && p.merge_frac > 0.0 && p.merge_frac < 1.0 && (p.swap == 0 || p.swap == 1) &&
                      (p.dir[0] == 1 || p.dir[0] == -1) && (p.dir[1] == 1 || p.dir[1] == -1),
                  "cpe_grid_relabel_batch: bad CpeRelabelParams (min_pts >= 2, 0 < merge_frac < 1, swap 0 or 1, dir +-1)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(xy && id && cnt && center && xy_out && id_out && cnt_out && src && lines && line_p && pitch && counts && flags,
                  "cpe_grid_relabel_batch: null pointer");
    {
        const size_t N = (size_t)n, P = (size_t)CPE_MAXP, L = (size_t)CPE_MAXL;
        const struct { const void *p; size_t bytes; } buf[13] = {
            {xy, N * P * 16}, {id, N * P * 8}, {cnt, N * 4}, {center, N * 16},
            {xy_out, N * P * 16}, {id_out, N * P * 8}, {cnt_out, N * 4}, {src, N * P * 4}, {lines, N * 2 * L * 16}, {line_p, N * 2 * L * 8},
            {pitch, N * 16}, {counts, N * 32}, {flags, N * 4}};
        for (int o = 4; o < 13; o++)
            for (int i = 0; i < o; i++)
                CPE_CHECK_ARG(!rl_overlap(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes),
                              "cpe_grid_relabel_batch: an output overlaps an input or another output");
    }
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_grid_relabel, dim3(n), dim3(128), 0, (hipStream_t)stream, xy, id, cnt, center, p.swap, p.min_pts, p.merge_frac, p.dir[0],
                p.dir[1], xy_out, id_out, cnt_out, src, lines, line_p, pitch, counts, flags);
    CPE_CHECK_LAUNCH("k_grid_relabel");
    return CPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The grid a fitted cylinder predicts, and the detections re-numbered against it (include/cpe.h cpe_grid_predict_batch and
// cpe_grid_assign_batch, whose numbered rules these follow).
namespace {

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// step 10 for one camera: -> visible; x, y are set for a visible node only
__device__ __forceinline__ bool pred_project(const double *__restrict__ K, const double *__restrict__ Tc, const double *X, const double *nu,
                                             double min_cos, int img_w, int img_h, double &x, double &y)
{
    TriCam cam;
    tri_cam(K, Tc, cam);
    double Xc[3] = {X[0], X[1], X[2]};
    if (Tc) {
#pragma unroll
        for (int r = 0; r < 3; r++) Xc[r] = ((Tc[4 * r] * X[0] + Tc[4 * r + 1] * X[1]) + Tc[4 * r + 2] * X[2]) + Tc[4 * r + 3];
    }
    const double Z = Xc[2];
    const double v[3] = {cam.o[0] - X[0], cam.o[1] - X[1], cam.o[2] - X[2]};
    const double vn = sqrt(dot3(v, v));
    if (!(Z > 0) || !(dot3(nu, v) > min_cos * vn)) return false;
    const double xn = Xc[0] / Z, yn = Xc[1] / Z;
    x = (cam.k0 * xn + cam.k1 * yn) + cam.k2;
    y = cam.k4 * yn + cam.k5;
    if (!isfinite(x) || !isfinite(y)) return false;
    if (img_w > 0 && img_h > 0 && !(x >= 0 && x < (double)img_w && y >= 0 && y < (double)img_h)) return false;
    return true;
}

// One lane per (frame, node): a block lies inside one frame, so the pose, the cameras and the centre are wave-uniform loads; the two
// planes of a node come through L2 as in k_table_triangulate.  Every output slot of the node is written, by vector stores.
__global__ __launch_bounds__(256) void k_grid_predict(const double *__restrict__ cyl, const unsigned char *__restrict__ use, double R,
                                                      const double *__restrict__ K1, const double *__restrict__ K2,
                                                      const double *__restrict__ T21, const double *__restrict__ P,
                                                      const int *__restrict__ line_status, int lo, int L,
                                                      const double *__restrict__ centre, int wlo0, int wlo1, int Nv, int N,
                                                      double min_cos, int img_w, int img_h, double *__restrict__ o_X,
                                                      double *__restrict__ o_px, int *__restrict__ o_state, int *__restrict__ o_vis)
{
    const int nb = (N + 255) / 256;                                            // blocks per frame: the grid is (frame, block) in one dimension
    const int f = blockIdx.x / nb;
    const int j = (blockIdx.x % nb) * 256 + threadIdx.x;
    if (j >= N) return;
    const double *c6 = cyl + (size_t)f * 6;
    const double oc[3] = {c6[0], c6[1], c6[2]};
    double ah[3] = {c6[3], c6[4], c6[5]};
    const double an = sqrt(dot3(ah, ah));
    bool frame_ok = (!use || use[f] != 0) && isfinite(oc[0]) && isfinite(oc[1]) && isfinite(oc[2]) && isfinite(ah[0]) &&
                    isfinite(ah[1]) && isfinite(ah[2]) && isfinite(an) && an != 0.0;
    int state = CPE_PRED_OK, vis = 0;
    double X[3] = {0, 0, 0}, px[4] = {0, 0, 0, 0};
    if (!frame_ok) state = CPE_PRED_NO_FRAME;
    if (state == CPE_PRED_OK) {
        const int l0 = (wlo0 + j / Nv) - lo, l1 = L + ((wlo1 + j % Nv) - lo);     // inside the table: checked by the host
        if (line_status[l0] != CPE_ST_OK || line_status[l1] != CPE_ST_OK) state = CPE_PRED_NO_PLANE;
        if (state == CPE_PRED_OK) {
#pragma unroll
            for (int a = 0; a < 3; a++) ah[a] = ah[a] / an;
            const double n0[3] = {P[(size_t)l0 * 4], P[(size_t)l0 * 4 + 1], P[(size_t)l0 * 4 + 2]}, p0 = P[(size_t)l0 * 4 + 3];
            const double n1[3] = {P[(size_t)l1 * 4], P[(size_t)l1 * 4 + 1], P[(size_t)l1 * 4 + 2]}, p1 = P[(size_t)l1 * 4 + 3];
            double w[3], c1[3], c0[3];
            cross3(n0, n1, w);
            const double w2 = dot3(w, w);
            if (!(w2 >= CPE_PRED_MIN_W2) || !isfinite(w2)) state = CPE_PRED_PARALLEL;
            if (state == CPE_PRED_OK) {
                cross3(n1, w, c1);
                cross3(w, n0, c0);
                const double wn = sqrt(w2);
                double q[3], wh[3], e[3], ep[3], wp[3];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    q[a] = ((-p0) * c1[a] - p1 * c0[a]) / w2;
                    wh[a] = w[a] / wn;
                    e[a] = q[a] - oc[a];
                }
                const double ea = dot3(e, ah), wa = dot3(wh, ah);
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    ep[a] = e[a] - ea * ah[a];
                    wp[a] = wh[a] - wa * ah[a];
                }
                const double A = dot3(wp, wp), B = dot3(ep, wp), Cq = dot3(ep, ep) - R * R;
                const double disc = B * B - A * Cq;
                if (!isfinite(A) || !isfinite(B) || !isfinite(Cq) || !isfinite(disc) || A == 0.0 || !(disc > 0)) state = CPE_PRED_MISS;
                if (state == CPE_PRED_OK) {
                    const double s = sqrt(disc);
                    const double tm = (-B - s) / A, tp = (-B + s) / A;
                    const double cq[3] = {centre[0] - q[0], centre[1] - q[1], centre[2] - q[2]};
                    const double tC = dot3(cq, wh);
                    const double t = fabs(tm - tC) <= fabs(tp - tC) ? tm : tp;
                    double g[3], nu[3], Xn[3];
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        Xn[a] = q[a] + t * wh[a];
                        g[a] = Xn[a] - oc[a];
                    }
                    if (!isfinite(Xn[0]) || !isfinite(Xn[1]) || !isfinite(Xn[2])) state = CPE_PRED_MISS;
                    if (state == CPE_PRED_OK) {
                        const double ga = dot3(g, ah);
#pragma unroll
                        for (int a = 0; a < 3; a++) nu[a] = (g[a] - ga * ah[a]) / R;
                        if (!(fabs(dot3(nu, wh)) >= min_cos)) state = CPE_PRED_GRAZING;
                        if (state == CPE_PRED_OK) {
#pragma unroll
                            for (int a = 0; a < 3; a++) X[a] = Xn[a];
                            double x, y;
                            if (pred_project(K1, nullptr, X, nu, min_cos, img_w, img_h, x, y)) { vis |= 1; px[0] = x; px[1] = y; }
                            if (pred_project(K2, T21, X, nu, min_cos, img_w, img_h, x, y)) { vis |= 2; px[2] = x; px[3] = y; }
                        }
                    }
                }
            }
        }
    }
    const size_t node = (size_t)f * N + j;
    o_X[node * 3] = X[0]; o_X[node * 3 + 1] = X[1]; o_X[node * 3 + 2] = X[2];
    const size_t pb = (size_t)f * 2 * N;
    o_px[(pb + j) * 2] = px[0]; o_px[(pb + j) * 2 + 1] = px[1];
    o_px[(pb + N + j) * 2] = px[2]; o_px[(pb + N + j) * 2 + 1] = px[3];
    o_state[node] = state;
    o_vis[node] = vis;
}

// counts of a frame from what k_grid_predict wrote: one wavefront per frame, so no atomics
__global__ __launch_bounds__(64) void k_grid_predict_counts(const int *__restrict__ state, const int *__restrict__ vis, int N,
                                                            int *__restrict__ o_counts)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    int ok = 0, v1 = 0, v2 = 0, vb = 0;
    for (int j = lane; j < N; j += 64) {
        const int s = state[(size_t)f * N + j], v = vis[(size_t)f * N + j];
        ok += s == CPE_PRED_OK; v1 += v & 1; v2 += (v >> 1) & 1; vb += v == 3;
    }
    ok = wave_sum_i(ok); v1 = wave_sum_i(v1); v2 = wave_sum_i(v2); vb = wave_sum_i(vb);
    if (lane == 0) { o_counts[4 * f] = ok; o_counts[4 * f + 1] = v1; o_counts[4 * f + 2] = v2; o_counts[4 * f + 3] = vb; }
}

// One workgroup of four wavefronts per image.  Dynamic LDS (fit_dyn): the camera's predicted pixels in f64 (N x 16 B, NaN for a
// node that is not visible, so it is never the nearest), d1 per detection (MAXP x 8 B), the winning key per node (N x 8 B: the
// bit pattern of the non-negative d1, which orders as the number does), the winning slot per node (N x 4 B), the named node or
// the refusal per detection (MAXP x 4 B) and the wave counts of the compaction: 28 N + 12 MAXP + 64 B, 139328 B at N = 4096,
// 55 KB at the experiment's 33 x 33 nodes.  All lanes of a wave read the same node at a time: a broadcast, no bank conflict.
constexpr int ASSIGN_T = 256;
constexpr size_t assign_lds_bytes(int N) { return (size_t)N * 28 + (size_t)MAXP * 12 + 64; }
__global__ __launch_bounds__(ASSIGN_T) void k_grid_assign(const double *__restrict__ xy, const int *__restrict__ id, const int *__restrict__ cnt,
                                                          const double *__restrict__ px, long long px_stride, const int *__restrict__ vis,
                                                          int cam_bit, int wlo0, int wlo1, int Nv, int N, double tau, double ratio, int swap,
                                                          double *__restrict__ o_xy, int *__restrict__ o_id, int *__restrict__ o_src,
                                                          double *__restrict__ o_dist, int *__restrict__ o_m, int *__restrict__ o_counts,
                                                          double *__restrict__ o_stats, int *__restrict__ o_node_slot)
{
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(cnt[f], 0), MAXP);
    const size_t base = (size_t)f * MAXP;
    double *s_px = fit_dyn;                                                     // [N][2]
    double *s_d1 = s_px + (size_t)2 * N;                                        // [MAXP]
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(s_d1 + MAXP);   // [N]
    int *s_slot = reinterpret_cast<int *>(s_key + N);                           // [N]
    int *s_node = s_slot + N;                                                   // [MAXP]
    int *s_wave = s_node + MAXP;                                                // [16]
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int j = tid; j < N; j += ASSIGN_T) {
        const double x = px[(size_t)f * px_stride + 2 * j], y = px[(size_t)f * px_stride + 2 * j + 1];
        const bool v = ((vis[(size_t)f * N + j] >> cam_bit) & 1) && isfinite(x) && isfinite(y);
        s_px[2 * j] = v ? x : nan; s_px[2 * j + 1] = v ? y : nan;
        s_key[j] = ~0ull;
        s_slot[j] = INT_MAX;
    }
    __syncthreads();
    // steps 1 - 4: the nearest and second-nearest node of every detection, and its bid for the node
    for (int k = tid; k < n; k += ASSIGN_T) {
        const double x = xy[(base + k) * 2], y = xy[(base + k) * 2 + 1];
        double b1 = INFINITY, b2 = INFINITY;
        int j1 = -1;
        for (int j = 0; j < N; j++) {
            const double dx = x - s_px[2 * j], dy = y - s_px[2 * j + 1];
            const double d = dx * dx + dy * dy;
            if (d < b1) { b2 = b1; b1 = d; j1 = j; }
            else if (d < b2) b2 = d;
        }
        const double d1 = sqrt(b1), d2 = sqrt(b2);
        int node = j1;
        if (!isfinite(x) || !isfinite(y) || j1 < 0) node = -3;                  // -(its slot in counts)
        else if (d1 >= tau) node = -4;
        else if (d1 > ratio * d2) node = -5;
        s_node[k] = node;
        s_d1[k] = d1;
        if (node >= 0) atomicMin(&s_key[node], (unsigned long long)__double_as_longlong(d1));
    }
    __syncthreads();
    // step 5: among the bids with the winning d1, the lowest slot
    for (int k = tid; k < n; k += ASSIGN_T) {
        const int node = s_node[k];
        if (node >= 0 && s_key[node] == (unsigned long long)__double_as_longlong(s_d1[k])) atomicMin(&s_slot[node], k);
    }
    __syncthreads();
    // steps 6, 7: compaction in slot order, rounds of 256: a ballot per wave, the waves' counts through LDS, the base carried on
    const unsigned long long below = (1ull << lane) - 1ull;
    int m = 0, c_same = 0, c_new = 0, c_none = 0, c_far = 0, c_amb = 0, c_conf = 0, round = 0;
    double r2 = 0, rmax = 0;
    for (int k0 = 0; k0 < n; k0 += ASSIGN_T, round++) {
        const int k = k0 + tid;
        const bool in = k < n;
        const int node = in ? s_node[k] : -1;
        const bool kept = in && node >= 0 && s_slot[node] == k;
        const unsigned long long bal = __ballot(kept);
        int *sw = s_wave + (round & 1) * 4;
        if (lane == 0) sw[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < ASSIGN_T / 64; w++) {
            const int c = sw[w];
            before += w < wave ? c : 0;
            total += c;
        }
        c_none += in && node == -3; c_far += in && node == -4; c_amb += in && node == -5; c_conf += in && node >= 0 && !kept;
        if (kept) {
            const size_t slot = base + (size_t)(m + before + __popcll(bal & below));   // <= base + k: inside the image's table
            const double x = xy[(base + k) * 2], y = xy[(base + k) * 2 + 1], d1 = s_d1[k];
            const int u = wlo0 + node / Nv, v = wlo1 + node % Nv;
            const int i0 = swap ? v : u, i1 = swap ? u : v;
            o_xy[slot * 2] = x; o_xy[slot * 2 + 1] = y;
            o_id[slot * 2] = i0; o_id[slot * 2 + 1] = i1;
            o_src[slot] = k;
            o_dist[slot] = d1;
            const bool same = id[(base + k) * 2] == i0 && id[(base + k) * 2 + 1] == i1;
            c_same += same; c_new += !same;
            r2 = r2 + d1 * d1;
            rmax = fmax(rmax, d1);
        }
        m += total;
    }
    // the sums: every lane its own points in slot order, the xor-butterfly of the wave, then the four waves in order
    r2 = wave_sum(r2);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
    c_same = wave_sum_i(c_same); c_new = wave_sum_i(c_new); c_none = wave_sum_i(c_none); c_far = wave_sum_i(c_far);
    c_amb = wave_sum_i(c_amb); c_conf = wave_sum_i(c_conf);
    __syncthreads();                                                            // s_d1 and s_node are free now
    if (lane == 0) {
        s_d1[2 * wave] = r2; s_d1[2 * wave + 1] = rmax;
        int *sc = s_node + 8 * wave;
        sc[0] = c_same; sc[1] = c_new; sc[2] = c_none; sc[3] = c_far; sc[4] = c_amb; sc[5] = c_conf;
    }
    __syncthreads();
    if (tid == 0) {
        double t2 = 0, tmax = 0;
        int c[6] = {0, 0, 0, 0, 0, 0};
        for (int w = 0; w < ASSIGN_T / 64; w++) {
            t2 = t2 + s_d1[2 * w];
            tmax = fmax(tmax, s_d1[2 * w + 1]);
            for (int a = 0; a < 6; a++) c[a] += s_node[8 * w + a];
        }
        o_m[f] = m;
        o_counts[8 * f] = m;
        for (int a = 0; a < 6; a++) o_counts[8 * f + 1 + a] = c[a];
        o_counts[8 * f + 7] = 0;
        o_stats[2 * f] = m > 0 ? sqrt(t2 / (double)m) : 0.0;
        o_stats[2 * f + 1] = m > 0 ? tmax : 0.0;
    }
    if (o_node_slot)
        for (int j = tid; j < N; j += ASSIGN_T) o_node_slot[(size_t)f * N + j] = s_slot[j] == INT_MAX ? -1 : s_slot[j];
}
}  // namespace

extern "C" int32_t cpe_grid_predict_batch(const double *cyl, const uint8_t *use, int32_t n, double radius, const double *K1,
                                          const double *K2, const double *T21, const double *P, const int32_t *line_status, int32_t lo,
                                          int32_t hi, const double *centre, const CpeGridPredictParams *params, double *X, double *px,
                                          int32_t *state, int32_t *vis, int32_t *counts, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_grid_predict_batch: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_grid_predict_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CPE_CHECK_ARG(radius > 0 && radius <= DBL_MAX, "cpe_grid_predict_batch: radius must be positive and finite");
    CpeGridPredictParams p = {{lo, lo}, {hi, hi}, 0.1, 0, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.min_cos > 0 && p.min_cos < 1, "cpe_grid_predict_batch: min_cos must lie in (0, 1)");
    for (int k = 0; k < 2; k++)
        CPE_CHECK_ARG(p.win_lo[k] >= lo && p.win_hi[k] <= hi && p.win_lo[k] <= p.win_hi[k],
                      "cpe_grid_predict_batch: the window of family %d, [%d, %d], must lie inside [%d, %d]", k, p.win_lo[k], p.win_hi[k], lo, hi);
    const long long Nu = (long long)p.win_hi[0] - p.win_lo[0] + 1, Nv = (long long)p.win_hi[1] - p.win_lo[1] + 1;
    CPE_CHECK_ARG(Nu * Nv <= CPE_PRED_MAXN, "cpe_grid_predict_batch: %lld x %lld nodes, at most %d", Nu, Nv, CPE_PRED_MAXN);
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(cyl && K1 && K2 && T21 && P && line_status && centre && X && px && state && vis && counts,
                  "cpe_grid_predict_batch: null pointer");
    const int N = (int)(Nu * Nv);
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_grid_predict, dim3((unsigned)((N + 255) / 256) * (unsigned)n), dim3(256), 0, (hipStream_t)stream, cyl, use, radius, K1, K2, T21, P, line_status, lo,
                hi - lo + 1, centre, p.win_lo[0], p.win_lo[1], (int)Nv, N, p.min_cos, p.img_w, p.img_h, X, px, state, vis);
    CPE_CHECK_LAUNCH("k_grid_predict");
    CPE_KLAUNCH(k_grid_predict_counts, dim3(n), dim3(64), 0, (hipStream_t)stream, (const int *)state, (const int *)vis, N, counts);
    CPE_CHECK_LAUNCH("k_grid_predict_counts");
    return CPE_OK;
}

extern "C" int32_t cpe_grid_assign_batch(const double *xy, const int32_t *id, const int32_t *cnt, int32_t n, const double *px,
                                         int64_t px_stride, const int32_t *vis, int32_t cam_bit, int32_t win_lo0, int32_t win_lo1,
                                         int32_t Nu, int32_t Nv, const CpeGridAssignParams *params, double *xy_out, int32_t *id_out,
                                         int32_t *src, double *dist, int32_t *m, int32_t *counts, double *stats, int32_t *node_slot,
                                         void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_grid_assign_batch: n < 0");
    CPE_CHECK_ARG(Nu >= 1 && Nv >= 1 && (long long)Nu * Nv <= CPE_PRED_MAXN, "cpe_grid_assign_batch: Nu x Nv must be 1..%d nodes",
                  CPE_PRED_MAXN);
    const int N = Nu * Nv;
    CPE_CHECK_ARG(px_stride >= 2 * (int64_t)N, "cpe_grid_assign_batch: px_stride below 2 N");
    CPE_CHECK_ARG(cam_bit == 0 || cam_bit == 1, "cpe_grid_assign_batch: cam_bit is 0 or 1");
    CPE_CHECK_ARG((long long)win_lo0 + Nu - 1 <= INT32_MAX && (long long)win_lo1 + Nv - 1 <= INT32_MAX,
                  "cpe_grid_assign_batch: the window's indices leave int32");
    CpeGridAssignParams p = {4.0, 0.5, 0, 0};
    if (params) p = *params;
    CPE_CHECK_ARG(p.tau_px > 0 && p.tau_px <= DBL_MAX && p.ratio > 0 && p.ratio <= 1 && (p.swap == 0 || p.swap == 1),
                  "cpe_grid_assign_batch: bad CpeGridAssignParams (tau_px positive and finite, 0 < ratio <= 1, swap 0 or 1)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(xy && id && cnt && px && vis && xy_out && id_out && src && dist && m && counts && stats,
                  "cpe_grid_assign_batch: null pointer");
    {
        const size_t Nn = (size_t)n, Pp = (size_t)CPE_MAXP;
        const struct { const void *p; size_t bytes; } buf[13] = {
            {xy, Nn * Pp * 16}, {id, Nn * Pp * 8}, {cnt, Nn * 4}, {px, ((Nn - 1) * (size_t)px_stride + 2 * (size_t)N) * 8}, {vis, Nn * N * 4},
            {xy_out, Nn * Pp * 16}, {id_out, Nn * Pp * 8}, {src, Nn * Pp * 4}, {dist, Nn * Pp * 8}, {m, Nn * 4}, {counts, Nn * 32},
            {stats, Nn * 16}, {node_slot, node_slot ? Nn * N * 4 : 0}};
        for (int o = 5; o < 13; o++)
            for (int i = 0; i < o; i++)
                CPE_CHECK_ARG(!buf[o].bytes || !rl_overlap(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes),
                              "cpe_grid_assign_batch: an output overlaps an input or another output");
    }
    static_assert(assign_lds_bytes(CPE_PRED_MAXN) <= 160 * 1024, "k_grid_assign: LDS beyond the CU's 160 KB");
    CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_grid_assign), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)assign_lds_bytes(CPE_PRED_MAXN)));
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_grid_assign, dim3(n), dim3(ASSIGN_T), assign_lds_bytes(N), (hipStream_t)stream, xy, id, cnt, px, (long long)px_stride, vis,
                cam_bit, win_lo0, win_lo1, Nv, N, p.tau_px, p.ratio, p.swap, xy_out, id_out, src, dist, m, counts, stats, node_slot);
    CPE_CHECK_LAUNCH("k_grid_assign");
    return CPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// BUILD-DEFINED (include/cpe.h cpe_mono_shift_batch, whose numbered rule this follows): the grid-index shift of a ONE-camera
// frame.  A point of one ray and two planes is over-determined by one, so the two residuals of cpe_table_triangulate_batch
// measure whether the pair of indices is right: per candidate (d0, d1), the points whose both residuals stay below tau vote.
// k_mono_vote: one wavefront per (frame, d0), lane l takes points l, l + 64, ...  The ray and the plane of component 0 (one
// plane per point, read through L2 as in k_table_triangulate) are made once per point; the family of component 1, which the
// inner loop over d1 reads 2 win1 + 1 times per point, is staged in LDS (at most 256 planes and statuses, 9 KB).  The cut is
// tri_cut itself, so a vote is decided by the bits cpe_table_triangulate_batch would write; the terms of component 0 are
// the same expressions in every unrolled d1 and are computed once.  The counts are ballots, uniform over the wavefront, behind
// a loop unrolled over the compile-time 17 candidates and predicated on |d1| <= win1 (no indexed register array).
// k_mono_pick: one wavefront per frame ranks the at most 289 counts by 64-bit keys, writes the first top_k, and walks the points
// once more for the residuals at the winner and at (0, 0).
namespace {

constexpr int MONO_SLOTS = (SHIFT_NC * SHIFT_NC + 63) / 64;       // candidates a lane of k_mono_pick holds

// step 3 for one point and one candidate: both planes cut with the ray; -> the point counts; rs = res[0], res[1]
__device__ __forceinline__ bool mono_counts(const double *o, const double *d, const double (*pl)[4], double min_sin2, double tau, double *rs)
{
    double X[3];
    bool early;
    rs[0] = 0; rs[1] = 0;
    return tri_cut(o, d, pl, 3, true, 1, min_sin2, 0.0, X, rs, early) && fabs(rs[0]) < tau && fabs(rs[1]) < tau;
}

// the plane of line r of the family that starts at line `fam` of the table -> usable; pl is loaded for a usable plane only
__device__ __forceinline__ bool mono_plane(const double *__restrict__ P, const int *__restrict__ line_status, size_t fam, int L, int r,
                                           double *pl)
{
    if (r < 0 || r >= L || line_status[fam + r] != CPE_ST_OK) return false;
#pragma unroll
    for (int a = 0; a < 4; a++) pl[a] = P[(fam + r) * 4 + a];
    return true;
}

__global__ __launch_bounds__(64) void k_mono_vote(const double *__restrict__ xy, const int *__restrict__ id, const int *__restrict__ cnt,
                                                  const double *__restrict__ K, const double *__restrict__ Tc,
                                                  const double *__restrict__ P, const int *__restrict__ line_status, int lo, int hi,
                                                  int win0, int win1, int swap, double min_sin2, double tau, int *__restrict__ o_scores)
{
    __shared__ double sP[CPE_MAXL * 4];
    __shared__ int sS[CPE_MAXL];
    const int n0 = 2 * win0 + 1, n1 = 2 * win1 + 1;       // win0, win1 in 0..SHIFT_W, checked by the host
    const int f = blockIdx.x / n0, d0 = (int)(blockIdx.x % n0) - win0, lane = threadIdx.x;
    const int n = min(max(cnt[f], 0), MAXP);
    const int L = hi - lo + 1;                            // 1..CPE_MAXL, checked by the host
    const size_t base = (size_t)f * MAXP;
    const size_t fam0 = (size_t)(swap * L), fam1 = (size_t)((1 ^ swap) * L);
    for (int i = lane; i < 4 * L; i += 64) sP[i] = P[fam1 * 4 + i];
    for (int i = lane; i < L; i += 64) sS[i] = line_status[fam1 + i];
    __syncthreads();
    TriCam cam;
    tri_cam(K, Tc, cam);
    // rel = id - lo of a point that can count at all lies in [-win, L - 1 + win]: tested in 64 bits, before any addition
    const long long hi0 = (long long)(L - 1 + win0), hi1 = (long long)(L - 1 + win1);
    int sc[SHIFT_NC];
#pragma unroll
    for (int j = 0; j < SHIFT_NC; j++) sc[j] = 0;
    for (int k0p = 0; k0p < n; k0p += 64) {
        const int k = k0p + lane;
        bool ok = k < n;
        double d[3] = {0, 0, 1}, pl[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        int rel1 = 0;
        if (ok) {
            const double x = xy[(base + k) * 2], y = xy[(base + k) * 2 + 1];
            const long long rl0 = (long long)id[(base + k) * 2] - (long long)lo, rl1 = (long long)id[(base + k) * 2 + 1] - (long long)lo;
            ok = isfinite(x) && isfinite(y) && rl0 >= -(long long)win0 && rl0 <= hi0 && rl1 >= -(long long)win1 && rl1 <= hi1;
            if (ok) ok = mono_plane(P, line_status, fam0, L, (int)rl0 + d0, pl[0]);
            if (ok) {
                tri_ray(cam, x, y, d);
                rel1 = (int)rl1;
            }
        }
#pragma unroll
        for (int j = 0; j < SHIFT_NC; j++) {
            if (abs(j - SHIFT_W) > win1) continue;        // (uniform)
            const int r1 = rel1 + (j - SHIFT_W);
            bool hit = false;
            if (ok && r1 >= 0 && r1 < L && sS[r1] == CPE_ST_OK) {
                double rs[2];
#pragma unroll
                for (int a = 0; a < 4; a++) pl[1][a] = sP[4 * r1 + a];
                hit = mono_counts(cam.o, d, pl, min_sin2, tau, rs);
            }
            sc[j] += __popcll(__ballot(hit));
        }
    }
    int mine = 0;
#pragma unroll
    for (int j = 0; j < SHIFT_NC; j++)
        if (lane == j) mine = sc[j];
    if (lane >= SHIFT_W - win1 && lane <= SHIFT_W + win1)
        o_scores[((size_t)f * n0 + (size_t)(d0 + win0)) * n1 + (lane - (SHIFT_W - win1))] = mine;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long u = __shfl_xor(v, off, 64);
        v = u < v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void k_mono_pick(const double *__restrict__ xy, const int *__restrict__ id, const int *__restrict__ cnt,
                                                  const double *__restrict__ K, const double *__restrict__ Tc,
                                                  const double *__restrict__ P, const int *__restrict__ line_status, int lo, int hi,
                                                  int win0, int win1, int swap, double min_sin2, double tau, int min_score, int top_k,
                                                  const int *__restrict__ scores, int *__restrict__ o_cand, int *__restrict__ o_cand_score,
                                                  int *__restrict__ o_score, double *__restrict__ o_rms, int *__restrict__ o_flags)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n1 = 2 * win1 + 1, C = (2 * win0 + 1) * n1;                 // 1..SHIFT_NC^2
    const int *sf = scores + (size_t)f * C;
    // the order of step 5 as one integer, smaller first: 2 MAXP - score | |d0| + |d1| | |d0| | d0 + 8 | d1 + 8; every candidate
    // has a key of its own and none is 0
    unsigned long long key[MONO_SLOTS];
#pragma unroll
    for (int i = 0; i < MONO_SLOTS; i++) {
        const int c = lane + 64 * i;
        key[i] = ~0ull;
        if (c < C) {
            const int d0 = c / n1 - win0, d1 = c % n1 - win1;
            const unsigned lowk = ((unsigned)(abs(d0) + abs(d1)) << 24) | ((unsigned)abs(d0) << 16) | ((unsigned)(d0 + SHIFT_W) << 8) |
                                  (unsigned)(d1 + SHIFT_W);
            key[i] = ((unsigned long long)(2 * MAXP - sf[c]) << 32) | lowk;
        }
    }
    int best = 0, second = 0, bd0 = 0, bd1 = 0;
    unsigned long long last = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        if (r >= max(top_k, 2)) break;                                     // (uniform; top_k in 1..8, checked by the host)
        unsigned long long m = ~0ull;
#pragma unroll
        for (int i = 0; i < MONO_SLOTS; i++)
            if (key[i] > last && key[i] < m) m = key[i];
        m = wave_min_u64(m);
        const bool any = m != ~0ull;
        const int s = any ? 2 * MAXP - (int)(m >> 32) : -1;
        const int d0 = any ? (int)((m >> 8) & 0xff) - SHIFT_W : 0, d1 = any ? (int)(m & 0xff) - SHIFT_W : 0;
        if (r == 0) { best = s; bd0 = d0; bd1 = d1; }
        if (r == 1) second = any ? s : 0;
        if (lane == 0 && r < top_k) {
            o_cand[((size_t)f * top_k + r) * 2] = d0; o_cand[((size_t)f * top_k + r) * 2 + 1] = d1;
            o_cand_score[(size_t)f * top_k + r] = s;
        }
        if (any) last = m;
    }
    const int at0 = sf[win0 * n1 + win1];
    // the counted points' squared residuals at the winner and at (0, 0)
    const int n = min(max(cnt[f], 0), MAXP);
    const int L = hi - lo + 1;
    const size_t base = (size_t)f * MAXP;
    const size_t fam0 = (size_t)(swap * L), fam1 = (size_t)((1 ^ swap) * L);
    const long long hi0 = (long long)(L - 1 + win0), hi1 = (long long)(L - 1 + win1);
    TriCam cam;
    tri_cam(K, Tc, cam);
    double sa = 0.0, s0 = 0.0;
    int ca = 0, c0 = 0, usable = 0;
    for (int k = lane; k < n; k += 64) {
        const double x = xy[(base + k) * 2], y = xy[(base + k) * 2 + 1];
        if (!(isfinite(x) && isfinite(y))) continue;
        usable++;
        const long long rl0 = (long long)id[(base + k) * 2] - (long long)lo, rl1 = (long long)id[(base + k) * 2 + 1] - (long long)lo;
        if (rl0 < -(long long)win0 || rl0 > hi0 || rl1 < -(long long)win1 || rl1 > hi1) continue;
        double d[3], pl[2][4], rs[2];
        tri_ray(cam, x, y, d);
        if (mono_plane(P, line_status, fam0, L, (int)rl0 + bd0, pl[0]) && mono_plane(P, line_status, fam1, L, (int)rl1 + bd1, pl[1]) &&
            mono_counts(cam.o, d, pl, min_sin2, tau, rs)) {
            sa = sa + (rs[0] * rs[0] + rs[1] * rs[1]);
            ca++;
        }
        if (mono_plane(P, line_status, fam0, L, (int)rl0, pl[0]) && mono_plane(P, line_status, fam1, L, (int)rl1, pl[1]) &&
            mono_counts(cam.o, d, pl, min_sin2, tau, rs)) {
            s0 = s0 + (rs[0] * rs[0] + rs[1] * rs[1]);
            c0++;
        }
    }
    sa = wave_sum(sa); s0 = wave_sum(s0); ca = wave_sum_i(ca); c0 = wave_sum_i(c0); usable = wave_sum_i(usable);
    if (lane == 0) {
        int flags = 0;
        if ((win0 > 0 && abs(bd0) == win0) || (win1 > 0 && abs(bd1) == win1)) flags |= CPE_SHIFT_FLAG_EDGE;
        if (best < min_score || best < 2 * second) flags |= CPE_SHIFT_FLAG_WEAK;
        o_score[4 * (size_t)f] = best; o_score[4 * (size_t)f + 1] = second; o_score[4 * (size_t)f + 2] = at0; o_score[4 * (size_t)f + 3] = usable;
        o_rms[2 * (size_t)f] = ca > 0 ? sqrt(sa / (double)ca) : 0.0;
        o_rms[2 * (size_t)f + 1] = c0 > 0 ? sqrt(s0 / (double)c0) : 0.0;
        o_flags[f] = flags;
    }
}
}  // namespace

extern "C" int32_t cpe_mono_shift_batch(const double *xy, const int32_t *id, const int32_t *cnt, int32_t n, const double *K,
                                        const double *Tc, const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                        int32_t win0, int32_t win1, double tau, double min_sin, int32_t min_score, int32_t swap,
                                        int32_t top_k, int32_t *scores, int32_t *cand, int32_t *cand_score,
                                        int32_t *score, double *rms, int32_t *flags, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_mono_shift_batch: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_mono_shift_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    const struct { int win[2]; double tau, min_sin; int min_score, swap, top_k; } p = {{win0, win1}, tau, min_sin, min_score, swap, top_k};
    CPE_CHECK_ARG(p.win[0] >= 0 && p.win[0] <= CPE_SHIFT_MAX_WIN && p.win[1] >= 0 && p.win[1] <= CPE_SHIFT_MAX_WIN,
                  "cpe_mono_shift_batch: window must be 0..%d for both components", CPE_SHIFT_MAX_WIN);
    CPE_CHECK_ARG(p.tau > 0 && p.min_sin >= 0 && p.min_score >= 0 && (p.swap == 0 || p.swap == 1) && p.top_k >= 1 && p.top_k <= 8,
                  "cpe_mono_shift_batch: bad parameters (tau > 0, min_sin >= 0, min_score >= 0, swap 0 or 1, top_k 1..8)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(xy && id && cnt && K && P && line_status && scores && cand && cand_score && score && rms && flags,
                  "cpe_mono_shift_batch: null pointer");
    const int L = hi - lo + 1, n0 = 2 * p.win[0] + 1, C = n0 * (2 * p.win[1] + 1);
    CPE_CHECK_ARG((long long)n * n0 <= INT_MAX, "cpe_mono_shift_batch: n (2 win[0] + 1) exceeds 2^31 - 1");
    {
        const size_t N = (size_t)n, Pp = (size_t)CPE_MAXP;
        const struct { const void *p; size_t bytes; } buf[13] = {
            {xy, N * Pp * 16}, {id, N * Pp * 8}, {cnt, N * 4}, {K, 72}, {Tc, Tc ? (size_t)128 : 0}, {P, (size_t)L * 64},
            {line_status, (size_t)L * 8},
            {scores, N * C * 4}, {cand, N * p.top_k * 8}, {cand_score, N * p.top_k * 4}, {score, N * 16}, {rms, N * 16}, {flags, N * 4}};
        for (int o = 7; o < 13; o++)
            for (int i = 0; i < o; i++)
                CPE_CHECK_ARG(!buf[i].bytes || !rl_overlap(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes),
                              "cpe_mono_shift_batch: an output overlaps an input or another output");
    }
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_mono_vote, dim3((unsigned)n * (unsigned)n0), dim3(64), 0, (hipStream_t)stream, xy, id, cnt, K, Tc, P, line_status, lo, hi,
                p.win[0], p.win[1], p.swap, p.min_sin * p.min_sin, p.tau, scores);
    CPE_CHECK_LAUNCH("k_mono_vote");
    CPE_KLAUNCH(k_mono_pick, dim3(n), dim3(64), 0, (hipStream_t)stream, xy, id, cnt, K, Tc, P, line_status, lo, hi, p.win[0], p.win[1], p.swap,
                p.min_sin * p.min_sin, p.tau, p.min_score, p.top_k, (const int *)scores, cand, cand_score, score, rms, flags);
    CPE_CHECK_LAUNCH("k_mono_pick");
    return CPE_OK;
}

// ------------------------------------------------------------------------------------------ curvatures of every point
// [K, L] = estCurvatures(Pts3) for every point of every frame (estCurvatures.m, HOT LOOP E of SURVEY.md), and what a frame's
// curvatures say together (build-defined).  The rule is in include/cpe.h at cpe_est_curvatures_batch.
//   k_est_curvatures       : one lane per point, 256 points per workgroup.  The frame's points are staged in LDS once; every lane
//                            scans them through broadcast reads and keeps its KM best (d2, index) pairs sorted in registers (a
//                            fully unrolled compare-and-shift: no dynamic register index).  The ranked list then goes to LDS as
//                            16-bit indices, column-per-lane, so that the algebra can walk it with a run-time count.  The algebra
//                            of mode 0 restates fit_init's block line by line (fit_init itself is left alone: its kernels must
//                            not change a bit), so for the point fit_init picks column 0 has the bits of cyl_raw[f,0,3:6].
//   k_curvature_consensus  : one wavefront per frame.
namespace {

constexpr int CURV_TPB = 256;
constexpr size_t CURV_LDS_BYTES = (size_t)MAXP * 3 * 8 + (size_t)CPE_CURV_MAXK * CURV_TPB * 2;

// MODE: CPE_CURV_REFERENCE / CPE_CURV_INTERCEPT; KM: length of the sorted list in registers (>= k)
template <int MODE, int KM>
__global__ __launch_bounds__(CURV_TPB) void k_est_curvatures(const double *__restrict__ X, const int *__restrict__ cnt, int kwant,
                                                             double *__restrict__ o_K, double *__restrict__ o_L,
                                                             double *__restrict__ o_normal, int *__restrict__ o_nbr,
                                                             unsigned char *__restrict__ o_pt, int *__restrict__ o_status)
{
    constexpr int NU = MODE == CPE_CURV_INTERCEPT ? 6 : 5;
    double *sP = fit_dyn;                                                         // [MAXP * 3]
    unsigned short *sNb = reinterpret_cast<unsigned short *>(sP + MAXP * 3);      // [CPE_CURV_MAXK][CURV_TPB]
    const int f = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * CURV_TPB + tid;
    const int n = min(max(cnt[f], 0), MAXP);
    const bool few = n < NU;
    if (p == 0) o_status[f] = few ? CPE_ST_FEW_POINTS : CPE_ST_OK;
    const size_t slot = (size_t)f * MAXP + p;
    double *oK = o_K + slot * 6, *oL = o_L + slot * 2, *oN = o_normal + slot * 3;
    int *oNb = o_nbr ? o_nbr + slot * kwant : nullptr;
    auto zero_slot = [&]() {
#pragma unroll
        for (int a = 0; a < 6; a++) oK[a] = 0.0;
        oL[0] = 0.0; oL[1] = 0.0;
        oN[0] = 0.0; oN[1] = 0.0; oN[2] = 0.0;
        if (oNb) for (int r = 0; r < kwant; r++) oNb[r] = 0;
    };
    if (few || blockIdx.x * CURV_TPB >= n) {   // the whole workgroup alike: nothing of it reaches a barrier
        zero_slot();
        o_pt[slot] = 0;
        return;
    }
    const double *Xf = X + (size_t)f * MAXP * 3;
    for (int i = tid; i < 3 * n; i += CURV_TPB) sP[i] = Xf[i];
    __syncthreads();
    if (p >= n) {
        zero_slot();
        o_pt[slot] = 0;
        return;
    }
    const int K = n < kwant ? n : kwant;

    // 1. the K nearest by (d2, index), the point itself included.  j ascends, so a candidate goes behind its equals.
    {
        double bd[KM];
        int bi[KM];
#pragma unroll
        for (int i = 0; i < KM; i++) { bd[i] = DBL_MAX; bi[i] = 0; }
        const double p0 = sP[3 * p], p1 = sP[3 * p + 1], p2 = sP[3 * p + 2];
        for (int j = 0; j < n; j++) {
            const double a = sP[3 * j] - p0, b = sP[3 * j + 1] - p1, c = sP[3 * j + 2] - p2;
            const double d = (a * a + b * b) + c * c;
            if (d < bd[KM - 1]) {
#pragma unroll
                for (int i = KM - 1; i >= 1; i--) {
                    const bool up = d < bd[i - 1], here = !up && d < bd[i];
                    bd[i] = up ? bd[i - 1] : (here ? d : bd[i]);
                    bi[i] = up ? bi[i - 1] : (here ? j : bi[i]);
                }
                if (d < bd[0]) { bd[0] = d; bi[0] = j; }
            }
        }
        // (a d2 that is NaN or +inf never enters the list: such a point is reported below through `listed`)
#pragma unroll
        for (int i = 0; i < KM; i++) sNb[i * CURV_TPB + tid] = (unsigned short)bi[i];
        int listed = 0;
#pragma unroll
        for (int i = 0; i < KM; i++) listed += (bd[i] < DBL_MAX) ? 1 : 0;
        if (oNb) {
#pragma unroll
            for (int i = 0; i < KM; i++)
                if (i < kwant) oNb[i] = (i < K && bd[i] < DBL_MAX) ? bi[i] : -1;
        }
        if (listed < K) {   // not finite coordinates in the frame
#pragma unroll
            for (int a = 0; a < 6; a++) oK[a] = 0.0;
            oL[0] = 0.0; oL[1] = 0.0;
            oN[0] = 0.0; oN[1] = 0.0; oN[2] = 0.0;
            o_pt[slot] = 1;
            return;
        }
    }
#define CURV_NB(k) ((int)sNb[(k) * CURV_TPB + tid])

    // 2. plane, local frame, quadric, 2 x 2 eigen-pair: fit_init's block, operation by operation
    double mu[3] = {0, 0, 0};
    for (int k = 0; k < K; k++) {
        const int q = CURV_NB(k);
        for (int c = 0; c < 3; c++) mu[c] = mu[c] + sP[3 * q + c];
    }
    for (int c = 0; c < 3; c++) mu[c] = mu[c] / (double)K;
    double C2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < K; k++) {
        const int q = CURV_NB(k);
        double e[3] = {sP[3 * q] - mu[0], sP[3 * q + 1] - mu[1], sP[3 * q + 2] - mu[2]};
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) C2[a * 3 + b] = C2[a * 3 + b] + e[a] * e[b];
    }
#pragma unroll
    for (int a = 0; a < 9; a++) C2[a] = C2[a] / (double)(K - 1);
    double w[3], V[9];
    eig3(C2, w, V);
    double z[3] = {V[0], V[3], V[6]};
    if (z[2] < 0) { z[0] = -z[0]; z[1] = -z[1]; z[2] = -z[2]; }
    double x[3] = {1, 0, 0};
    if (fabs(z[0]) > 0.9) { x[0] = 0; x[1] = 1; }
    double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    if (MODE == CPE_CURV_INTERCEPT) {
        const double yn = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
        y[0] = y[0] / yn; y[1] = y[1] / yn; y[2] = y[2] / yn;
    }
    double xx[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
    double M[NU * NU], rhs[NU], co[NU];
#pragma unroll
    for (int a = 0; a < NU * NU; a++) M[a] = 0;
#pragma unroll
    for (int a = 0; a < NU; a++) rhs[a] = 0;
    for (int k = 0; k < K; k++) {
        const int q = CURV_NB(k);
        double e[3] = {sP[3 * q] - mu[0], sP[3 * q + 1] - mu[1], sP[3 * q + 2] - mu[2]};
        double lx = (e[0] * xx[0] + e[1] * xx[1]) + e[2] * xx[2];
        double ly = (e[0] * y[0] + e[1] * y[1]) + e[2] * y[2];
        double lz = (e[0] * z[0] + e[1] * z[1]) + e[2] * z[2];
        double row[NU];
        row[0] = lx * lx; row[1] = lx * ly; row[2] = ly * ly; row[3] = lx; row[4] = ly;
        if (MODE == CPE_CURV_INTERCEPT) row[NU - 1] = 1.0;
#pragma unroll
        for (int a = 0; a < NU; a++) {
#pragma unroll
            for (int b = 0; b < NU; b++) M[a * NU + b] = M[a * NU + b] + row[a] * row[b];
            rhs[a] = rhs[a] + row[a] * lz;
        }
    }
#undef CURV_NB
    bool ok = gauss_solve<NU>(M, rhs, co);
    double a = co[0] * 2, b = co[1], c = co[2] * 2;
    double hd = (a - c) / 2.0, mid = (a + c) / 2.0, rad = sqrt(hd * hd + b * b);
    double kd[6], lam[2] = {mid - rad, mid + rad};  // eig ascending: V(:,1), V(:,2)
#pragma unroll
    for (int j = 0; j < 2; j++) {
        double v0, v1;
        if (fabs(lam[j] - a) >= fabs(lam[j] - c)) { v0 = b; v1 = lam[j] - a; }
        else { v0 = lam[j] - c; v1 = b; }
        double nn = sqrt(v0 * v0 + v1 * v1);
        if (nn == 0) { v0 = j == 0 ? 1 : 0; v1 = j == 0 ? 0 : 1; nn = 1; }   // eig of a multiple of the identity: I
        v0 = v0 / nn;
        v1 = v1 / nn;
        for (int k = 0; k < 3; k++) kd[3 * j + k] = xx[k] * v0 + y[k] * v1;
    }
    ok = ok && isfinite(lam[0]) && isfinite(lam[1]) && isfinite(z[0]) && isfinite(z[1]) && isfinite(z[2]);
#pragma unroll
    for (int k = 0; k < 6; k++) ok = ok && isfinite(kd[k]);
#pragma unroll
    for (int k = 0; k < 6; k++) oK[k] = ok ? kd[k] : 0.0;
    oL[0] = ok ? lam[0] : 0.0;
    oL[1] = ok ? lam[1] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) oN[k] = ok ? z[k] : 0.0;
    o_pt[slot] = ok ? 0 : 1;
}

// what a frame's curvatures say together: the gate, the consensus direction, the centres of curvature, the median radius
__global__ __launch_bounds__(64) void k_curvature_consensus(const double *__restrict__ X, const int *__restrict__ cnt,
                                                            const double *__restrict__ Kdir, const double *__restrict__ Lam,
                                                            const double *__restrict__ normal, const unsigned char *__restrict__ pt,
                                                            double rho_max, double r_min, double r_max, double *__restrict__ o_axis,
                                                            int *__restrict__ o_ng, unsigned char *__restrict__ o_gate,
                                                            int *__restrict__ o_status)
{
    __shared__ unsigned long long sR[MAXP];   // bits of 1 / |lambda|max of a gated point, all ones otherwise
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(cnt[f], 0), MAXP);
    const double *Xf = X + (size_t)f * MAXP * 3, *Kf = Kdir + (size_t)f * MAXP * 6, *Lf = Lam + (size_t)f * MAXP * 2;
    const double *Nf = normal + (size_t)f * MAXP * 3;
    const unsigned char *ptf = pt + (size_t)f * MAXP;
    unsigned char *gf = o_gate + (size_t)f * MAXP;

    // pass 1: the gate; sums of t t' and of the centres of curvature
    double S[6] = {0, 0, 0, 0, 0, 0}, cs[3] = {0, 0, 0};
    int g = 0;
    for (int k = lane; k < MAXP; k += 64) {
        bool in = false;
        if (k < n && ptf[k] == 0) {
            const double l0 = Lf[2 * k], l1 = Lf[2 * k + 1];
            const double a0 = fabs(l0), a1 = fabs(l1);
            const int big = a1 > a0 ? 1 : 0;
            const double amax = big ? a1 : a0, amin = big ? a0 : a1, lbig = big ? l1 : l0;
            const double r = 1.0 / amax;
            const double *t = Kf + 6 * k + 3 * (1 - big);
            const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
            in = amax > 0 && amin / amax <= rho_max && r_min < r && r < r_max && tn > 0 && isfinite(tn) && isfinite(r);
            if (in) {
                const double t0 = t[0] / tn, t1 = t[1] / tn, t2 = t[2] / tn;
                S[0] = S[0] + t0 * t0; S[1] = S[1] + t0 * t1; S[2] = S[2] + t0 * t2;
                S[3] = S[3] + t1 * t1; S[4] = S[4] + t1 * t2; S[5] = S[5] + t2 * t2;
#pragma unroll
                for (int c = 0; c < 3; c++) cs[c] = cs[c] + (Xf[3 * k + c] + Nf[3 * k + c] / lbig);
                sR[k] = (unsigned long long)__double_as_longlong(r);
                g++;
            }
        }
        if (!in) sR[k] = ~0ull;
        gf[k] = in ? 1 : 0;
    }
    g = wave_sum_i(g);
#pragma unroll
    for (int a = 0; a < 6; a++) S[a] = wave_sum(S[a]);
#pragma unroll
    for (int c = 0; c < 3; c++) cs[c] = wave_sum(cs[c]);
    __syncthreads();

    double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = g >= 3;
    if (ok) {
        double org[3], dir[3];
#pragma unroll
        for (int c = 0; c < 3; c++) org[c] = cs[c] / (double)g;
        const double Sm[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]};
        double w[3], V[9];
        eig3(Sm, w, V);
        dir[0] = V[2]; dir[1] = V[5]; dir[2] = V[8];
        {   // the largest-magnitude component (the first of them) positive
            double m = fabs(dir[0]), s = dir[0];
            if (fabs(dir[1]) > m) { m = fabs(dir[1]); s = dir[1]; }
            if (fabs(dir[2]) > m) { m = fabs(dir[2]); s = dir[2]; }
            if (s < 0) { dir[0] = -dir[0]; dir[1] = -dir[1]; dir[2] = -dir[2]; }
        }
        // the lower median of the radii by exact selection: the bits of positive doubles order as the numbers do
        unsigned long long prefix = 0;
        int rank = (g - 1) / 2;
        for (int bit = 63; bit >= 0; bit--) {
            int c0 = 0;
            for (int k = lane; k < n; k += 64) c0 += ((sR[k] >> bit) == (prefix >> bit)) ? 1 : 0;
            c0 = wave_sum_i(c0);
            if (rank >= c0) { rank -= c0; prefix |= 1ull << bit; }
        }
        const double radius = __longlong_as_double((long long)prefix);
        // pass 2: rms distance of the centres of curvature from the line (org, dir)
        double acc = 0.0;
        for (int k = lane; k < n; k += 64) {
            if (sR[k] == ~0ull) continue;
            const double l0 = Lf[2 * k], l1 = Lf[2 * k + 1];
            const double lbig = fabs(l1) > fabs(l0) ? l1 : l0;
            double e[3];
#pragma unroll
            for (int c = 0; c < 3; c++) e[c] = (Xf[3 * k + c] + Nf[3 * k + c] / lbig) - org[c];
            const double al = (e[0] * dir[0] + e[1] * dir[1]) + e[2] * dir[2];
#pragma unroll
            for (int c = 0; c < 3; c++) e[c] = e[c] - dir[c] * al;
            acc = acc + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        }
        const double spread = sqrt(wave_sum(acc) / (double)g);
        out[0] = org[0]; out[1] = org[1]; out[2] = org[2];
        out[3] = dir[0]; out[4] = dir[1]; out[5] = dir[2];
        out[6] = radius; out[7] = spread;
#pragma unroll
        for (int a = 0; a < 8; a++) ok = ok && isfinite(out[a]);
    }
    if (lane < 8) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < 8; a++) v = (lane == a && ok) ? out[a] : v;
        o_axis[(size_t)f * 8 + lane] = v;
    }
    if (lane == 0) { o_ng[f] = g; o_status[f] = ok ? CPE_ST_OK : CPE_ST_FEW_POINTS; }
}
}  // namespace

extern "C" int32_t cpe_est_curvatures_batch(const double *X, const int32_t *cnt, int32_t n, int32_t k, int32_t mode, double *Kdir,
                                            double *L, double *normal, int32_t *nbr, uint8_t *pt_status, int32_t *status,
                                            void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_est_curvatures_batch: n < 0");
    const struct { int k, mode; } p = {k, mode};
    CPE_CHECK_ARG(p.mode == CPE_CURV_REFERENCE || p.mode == CPE_CURV_INTERCEPT, "cpe_est_curvatures_batch: unknown mode %d", p.mode);
    const int unknowns = p.mode == CPE_CURV_INTERCEPT ? 6 : 5;
    CPE_CHECK_ARG(p.k >= unknowns && p.k <= CPE_CURV_MAXK, "cpe_est_curvatures_batch: k = %d must be %d..%d in mode %d", p.k, unknowns,
                  CPE_CURV_MAXK, p.mode);
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(X && cnt && Kdir && L && normal && pt_status && status, "cpe_est_curvatures_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    const dim3 grid(MAXP / CURV_TPB, n), block(CURV_TPB);
#define CURV_LAUNCH(MODE, KM)                                                                                                       \
    do {                                                                                                                            \
        CPE_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_est_curvatures<MODE, KM>),                              \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)CURV_LDS_BYTES));                        \
        CPE_KLAUNCH((k_est_curvatures<MODE, KM>), grid, block, CURV_LDS_BYTES, (hipStream_t)stream, X, cnt, p.k, Kdir, L, normal, nbr, \
                    pt_status, status);                                                                                             \
    } while (0)
    if (p.mode == CPE_CURV_INTERCEPT) {
        if (p.k <= 20) CURV_LAUNCH(CPE_CURV_INTERCEPT, 20);
        else CURV_LAUNCH(CPE_CURV_INTERCEPT, CPE_CURV_MAXK);
    } else {
        if (p.k <= 20) CURV_LAUNCH(CPE_CURV_REFERENCE, 20);
        else CURV_LAUNCH(CPE_CURV_REFERENCE, CPE_CURV_MAXK);
    }
#undef CURV_LAUNCH
    CPE_CHECK_LAUNCH("k_est_curvatures");
    return CPE_OK;
}

extern "C" int32_t cpe_curvature_consensus_batch(const double *X, const int32_t *cnt, int32_t n, const double *Kdir, const double *L,
                                                 const double *normal, const uint8_t *pt_status, double rho_max, double r_min,
                                                 double r_max, double *axis, int32_t *n_gated, uint8_t *gate, int32_t *status,
                                                 void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_curvature_consensus_batch: n < 0");
    const struct { double rho_max, r_min, r_max; } g = {rho_max, r_min, r_max};
    CPE_CHECK_ARG(g.rho_max >= 0 && g.r_min >= 0 && g.r_max > g.r_min,
                  "cpe_curvature_consensus_batch: bad gate (rho_max >= 0, 0 <= r_min < r_max, none NaN)");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(X && cnt && Kdir && L && normal && pt_status && axis && n_gated && gate && status,
                  "cpe_curvature_consensus_batch: null pointer");
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_curvature_consensus, dim3(n), dim3(64), 0, (hipStream_t)stream, X, cnt, Kdir, L, normal, pt_status, g.rho_max, g.r_min,
                g.r_max, axis, n_gated, gate, status);
    CPE_CHECK_LAUNCH("k_curvature_consensus");
    return CPE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// BUILD-DEFINED (include/cpe.h cpe_fit_cylinder_pixels_batch, whose numbered rule this follows): the cylinder pose that minimises
// the PIXEL distance between every detection and the predicted pixel of its own grid node, in both images at once.
// k_fit_cylinder_pixels: one wavefront per frame.  The two table families and their statuses are staged in LDS once (16 L x 4 B
// + 2 L x 4 B, 18 KB at L = 256).  The detections are NOT staged: both tables are 98 KB per frame, which would leave one
// wavefront per CU; they are re-read on every pass (24 B per detection, coalesced, L2-resident after the first pass: a frame of
// 500 detections is 12 KB), and what a pass needs of a node (q, wh, tC: 60 flops from the two planes) is made again from LDS.
// Lane l owns the detections l, l + 64, ... of the concatenated list (camera 1's slots, then camera 2's): at most 64 of them, so
// membership of the used set S is one 64-bit register per lane, no LDS and no workspace.  Sums: every lane its own detections in
// that order, then wave_sum.  Steps 3 - 9 of the prediction are restated from k_grid_predict, which is left alone (its
// instructions may not change), as k_est_curvatures restated fit_init.
namespace {

// steps 3 - 9 of cpe_grid_predict_batch for the node of the planes pl0 (family 0) and pl1 (family 1) at the pose (oc, ah):
// -> CPE_PRED_*; X and wh are set for CPE_PRED_OK
__device__ __forceinline__ int pix_node(const double *pl0, const double *pl1, const double *oc, const double *ah, double R,
                                        const double *centre, double min_cos, double *X, double *wh)
{
    const double n0[3] = {pl0[0], pl0[1], pl0[2]}, p0 = pl0[3];
    const double n1[3] = {pl1[0], pl1[1], pl1[2]}, p1 = pl1[3];
    double w[3], c1[3], c0[3];
    cross3(n0, n1, w);
    const double w2 = dot3(w, w);
    if (!(w2 >= CPE_PRED_MIN_W2) || !isfinite(w2)) return CPE_PRED_PARALLEL;
    cross3(n1, w, c1);
    cross3(w, n0, c0);
    const double wn = sqrt(w2);
    double q[3], e[3], ep[3], wp[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        q[a] = ((-p0) * c1[a] - p1 * c0[a]) / w2;
        wh[a] = w[a] / wn;
        e[a] = q[a] - oc[a];
    }
    const double ea = dot3(e, ah), wa = dot3(wh, ah);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        ep[a] = e[a] - ea * ah[a];
        wp[a] = wh[a] - wa * ah[a];
    }
    const double A = dot3(wp, wp), B = dot3(ep, wp), Cq = dot3(ep, ep) - R * R;
    const double disc = B * B - A * Cq;
    if (!isfinite(A) || !isfinite(B) || !isfinite(Cq) || !isfinite(disc) || A == 0.0 || !(disc > 0)) return CPE_PRED_MISS;
    const double s = sqrt(disc);
    const double tm = (-B - s) / A, tp = (-B + s) / A;
    const double cq[3] = {centre[0] - q[0], centre[1] - q[1], centre[2] - q[2]};
    const double tC = dot3(cq, wh);
    const double t = fabs(tm - tC) <= fabs(tp - tC) ? tm : tp;
    double g[3], nu[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        X[a] = q[a] + t * wh[a];
        g[a] = X[a] - oc[a];
    }
    if (!isfinite(X[0]) || !isfinite(X[1]) || !isfinite(X[2])) return CPE_PRED_MISS;
    const double ga = dot3(g, ah);
#pragma unroll
    for (int a = 0; a < 3; a++) nu[a] = (g[a] - ga * ah[a]) / R;
    if (!(fabs(dot3(nu, wh)) >= min_cos)) return CPE_PRED_GRAZING;
    return CPE_PRED_OK;
}

// one detection's node at a pose: its point, the line's direction, the point in its camera and the residual (predicted - detected)
struct PixEval {
    double X[3], wh[3], Xc[3], r[2];
    int cam;
};

// one frame's detections against the table: what k_fit_cylinder_pixels and k_multi_frame_pixels share
struct PixFrame {
    const double *xy1, *xy2;       // the frame's two tables (a table of an absent camera is never read: its count is 0)
    const int *id1, *id2;
    int n1, n12;                   // camera 1's count; both counts
    const double *sP;              // LDS: P[2][L][4]
    const int *sSt;                // LDS: line_status[2][L]
    int lo, hi, L, swap;
    double R, min_cos;
    double centre[3];
    TriCam cam1, cam2;
    double t2[3];                  // camera 2's translation (camera 1's is 0)
    int lane;

    // a / |a| -> false: the pose cannot be used (rule 1)
    __device__ __forceinline__ static bool pose(const double *x, double *ah, double &an)
    {
        an = sqrt(dot3(x + 3, x + 3));
        bool ok = isfinite(an) && an != 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) ok = ok && isfinite(x[a]);
#pragma unroll
        for (int a = 0; a < 3; a++) ah[a] = x[3 + a] / an;
        return ok;
    }
    // camera c by selects: an index that differs between lanes would put both cameras into scratch memory
    __device__ __forceinline__ void camera(int c, TriCam &o) const
    {
#pragma unroll
        for (int a = 0; a < 9; a++) o.R[a] = c ? cam2.R[a] : cam1.R[a];
        o.k0 = c ? cam2.k0 : cam1.k0; o.k1 = c ? cam2.k1 : cam1.k1; o.k2 = c ? cam2.k2 : cam1.k2;
        o.k4 = c ? cam2.k4 : cam1.k4; o.k5 = c ? cam2.k5 : cam1.k5;
    }
    // rule 2's tests of the detection k of the concatenated list that do not depend on the pose -> its camera, pixel and planes
    __device__ __forceinline__ bool detection(int k, int &c, double &px, double &py, const double *&pl0, const double *&pl1) const
    {
        c = k >= n1;
        const int slot = c ? k - n1 : k;
        const double *p = (c ? xy2 : xy1) + (size_t)slot * 2;
        const int *v = (c ? id2 : id1) + (size_t)slot * 2;
        px = p[0]; py = p[1];
        const int u0 = v[swap], u1 = v[1 - swap];                          // the indices of table family 0 and 1
        if (u0 < lo || u0 > hi || u1 < lo || u1 > hi) return false;        // (compared, not subtracted: an index may be any int)
        const int l0 = u0 - lo, l1 = L + (u1 - lo);
        if (sSt[l0] != CPE_ST_OK || sSt[l1] != CPE_ST_OK) return false;
        pl0 = sP + 4 * l0; pl1 = sP + 4 * l1;
        return isfinite(px) && isfinite(py);
    }
    // the node of a detection that passed detection(), at the pose (oc, ah) -> it exists, lies before its camera, and its pixel is finite
    __device__ __forceinline__ bool eval(int c, double px, double py, const double *pl0, const double *pl1, const double *oc,
                                         const double *ah, PixEval &e) const
    {
        e.cam = c;
        if (pix_node(pl0, pl1, oc, ah, R, centre, min_cos, e.X, e.wh) != CPE_PRED_OK) return false;
        TriCam cm;
        camera(c, cm);
#pragma unroll
        for (int r = 0; r < 3; r++)
            e.Xc[r] = ((cm.R[3 * r] * e.X[0] + cm.R[3 * r + 1] * e.X[1]) + cm.R[3 * r + 2] * e.X[2]) + (c ? t2[r] : 0.0);
        const double Z = e.Xc[2];
        if (!(Z > 0)) return false;
        const double xn = e.Xc[0] / Z, yn = e.Xc[1] / Z;
        const double x = (cm.k0 * xn + cm.k1 * yn) + cm.k2;
        const double y = cm.k4 * yn + cm.k5;
        e.r[0] = x - px; e.r[1] = y - py;
        return isfinite(x) && isfinite(y);
    }
    __device__ __forceinline__ bool eval_k(int k, const double *oc, const double *ah, PixEval &e) const
    {
        int c;
        double px, py;
        const double *pl0, *pl1;
        return detection(k, c, px, py, pl0, pl1) && eval(c, px, py, pl0, pl1, oc, ah, e);
    }
    // rule 7's pieces of a node that eval() gave: u = gp / den, w = (g.ah) gp / (|a| den), and s = (d pi / d Xc) R_j wh
    __device__ __forceinline__ void node_derivatives(const PixEval &e, const double *oc, const double *ah, double an, double *dt,
                                                     double &sx, double &sy) const
    {
        const double gv[3] = {e.X[0] - oc[0], e.X[1] - oc[1], e.X[2] - oc[2]};
        const double ga = dot3(gv, ah);
        const double gp[3] = {gv[0] - ga * ah[0], gv[1] - ga * ah[1], gv[2] - ga * ah[2]};
        const double den = dot3(gp, e.wh);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            dt[a] = gp[a] / den;
            dt[3 + a] = ((ga * gp[a]) / an) / den;
        }
        TriCam cm;
        camera(e.cam, cm);
        double v[3];
#pragma unroll
        for (int r = 0; r < 3; r++) v[r] = (cm.R[3 * r] * e.wh[0] + cm.R[3 * r + 1] * e.wh[1]) + cm.R[3 * r + 2] * e.wh[2];
        const double Z = e.Xc[2], Z2 = Z * Z;
        sx = ((cm.k0 / Z) * v[0] + (cm.k1 / Z) * v[1]) + (-(cm.k0 * e.Xc[0] + cm.k1 * e.Xc[1]) / Z2) * v[2];
        sy = (cm.k4 / Z) * v[1] + (-(cm.k4 * e.Xc[1]) / Z2) * v[2];
    }
};

struct PixProblem : PixFrame {
    unsigned long long mine;       // bit i: the detection lane + 64 i belongs to S

    // rule 5
    __device__ __forceinline__ double operator()(const double *x) const
    {
        double ah[3], an, acc = 0.0;
        bool bad = !pose(x, ah, an);
        for (int i = 0, k = lane; k < n12; i++, k += 64) {
            if (!((mine >> i) & 1ull)) continue;
            PixEval e;
            if (!eval_k(k, x, ah, e)) { bad = true; continue; }
            acc = acc + (e.r[0] * e.r[0] + e.r[1] * e.r[1]);
        }
        acc = wave_sum(acc);
        return __ballot(bad) != 0ull ? __longlong_as_double(0x7ff8000000000000ll) : acc;
    }
    // rule 7: two rank-one rows per detection
    __device__ __forceinline__ void normal(const double *x, double *A, double *g) const
    {
        double acc[27], ah[3], an;
#pragma unroll
        for (int k = 0; k < 27; k++) acc[k] = 0.0;
        pose(x, ah, an);
        for (int i = 0, k = lane; k < n12; i++, k += 64) {
            if (!((mine >> i) & 1ull)) continue;
            PixEval e;
            if (!eval_k(k, x, ah, e)) continue;
            double dt[6], sx, sy;
            node_derivatives(e, x, ah, an, dt, sx, sy);
            double j[6];
#pragma unroll
            for (int a = 0; a < 6; a++) j[a] = sx * dt[a];
            normal_accumulate<6>(j, e.r[0], acc);
#pragma unroll
            for (int a = 0; a < 6; a++) j[a] = sy * dt[a];
            normal_accumulate<6>(j, e.r[1], acc);
        }
#pragma unroll
        for (int k = 0; k < 21; k++) A[k] = wave_sum(acc[k]);
#pragma unroll
        for (int k = 0; k < 6; k++) g[k] = wave_sum(acc[21 + k]);
    }
    __device__ __forceinline__ bool candidate(const double *x, const double *dl, double *xn) const
    {
#pragma unroll
        for (int k = 0; k < 6; k++) xn[k] = x[k] + dl[k];
        return true;
    }
};

struct PixOut {
    double *cyl, *fvals;
    int *iters, *counts;
    double *stats;
    int *status;
    double *res;                   // optional from here on
    int *pt_state;
    double *X;
};

__global__ __launch_bounds__(64) void k_fit_cylinder_pixels(const double *__restrict__ xy1, const int *__restrict__ id1,
                                                            const int *__restrict__ cnt1, const double *__restrict__ xy2,
                                                            const int *__restrict__ id2, const int *__restrict__ cnt2,
                                                            const double *__restrict__ cyl0, const unsigned char *__restrict__ use, double R,
                                                            const double *__restrict__ K1, const double *__restrict__ K2,
                                                            const double *__restrict__ T21, const double *__restrict__ P,
                                                            const int *__restrict__ line_status, int lo, int L,
                                                            const double *__restrict__ centre, int swap, double min_cos, double gate_px,
                                                            double tolx, double tolf, int maxiter, const PixOut out)
{
    __shared__ double sP[2 * CPE_MAXL * 4];
    __shared__ int sSt[2 * CPE_MAXL];
    const int f = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < 8 * L; i += 64) sP[i] = P[i];
    for (int i = lane; i < 2 * L; i += 64) sSt[i] = line_status[i];
    __syncthreads();
    const size_t tb = (size_t)f * MAXP * 2;
    PixProblem prob;
    prob.xy1 = xy1 ? xy1 + tb : nullptr; prob.xy2 = xy2 ? xy2 + tb : nullptr;
    prob.id1 = id1 ? id1 + tb : nullptr; prob.id2 = id2 ? id2 + tb : nullptr;
    const int n1 = xy1 ? min(max(cnt1[f], 0), MAXP) : 0, n2 = xy2 ? min(max(cnt2[f], 0), MAXP) : 0;
    prob.n1 = n1; prob.n12 = n1 + n2;
    prob.sP = sP; prob.sSt = sSt;
    prob.lo = lo; prob.hi = lo + (L - 1); prob.L = L; prob.swap = swap;
    prob.R = R; prob.min_cos = min_cos;
#pragma unroll
    for (int a = 0; a < 3; a++) { prob.centre[a] = centre[a]; prob.t2[a] = T21[4 * a + 3]; }
    tri_cam(K1, nullptr, prob.cam1);
    tri_cam(K2, T21, prob.cam2);
    prob.lane = lane;
    prob.mine = 0ull;

    // rule 1
    double x0[6], ah0[3], an0;
#pragma unroll
    for (int a = 0; a < 6; a++) x0[a] = cyl0[(size_t)f * 6 + a];
    const bool frame_ok = PixProblem::pose(x0, ah0, an0) && (!use || use[f] != 0);

    // rules 2, 3: the used set, once
    unsigned long long gated = 0ull;
    int c1 = 0, c2 = 0, c_ref = 0, c_gate = 0;
    double f0 = 0.0;
    if (frame_ok) {
        for (int i = 0, k = lane; k < prob.n12; i++, k += 64) {
            PixEval e;
            if (!prob.eval_k(k, x0, ah0, e)) { c_ref++; continue; }
            const double r2 = e.r[0] * e.r[0] + e.r[1] * e.r[1];
            if (gate_px > 0 && sqrt(r2) >= gate_px) { gated |= 1ull << i; c_gate++; continue; }
            prob.mine |= 1ull << i;
            c1 += k < n1; c2 += k >= n1;
            f0 = f0 + r2;
        }
        c1 = wave_sum_i(c1); c2 = wave_sum_i(c2); c_ref = wave_sum_i(c_ref); c_gate = wave_sum_i(c_gate);
        f0 = wave_sum(f0);
    }
    // rules 4, 6, 8
    double xf[6] = {0, 0, 0, 0, 0, 0}, ffinal = 0.0;
    int itercount = 0, func_evals = 0;
    bool ok = frame_ok && c1 + c2 >= CPE_PIXFIT_MIN_PTS;
    if (ok) {
        func_evals = 1;
        lm_minimize<6>(prob, x0, f0, tolx, tolf, maxiter, xf, ffinal, itercount, func_evals);
        ok = fit_finite(xf, ffinal);
    }
    // the outputs: every slot of the frame
    double ahf[3], anf, s1 = 0.0, s2 = 0.0, rmax = 0.0;
    if (ok) PixProblem::pose(xf, ahf, anf);
    for (int i = 0, k = lane; k < prob.n12; i++, k += 64) {
        const int c = k >= n1, slot = c ? k - n1 : k;
        const size_t at = ((size_t)f * 2 + c) * MAXP + slot;
        const bool used = (prob.mine >> i) & 1ull;
        double r[2] = {0, 0}, Xn[3] = {0, 0, 0};
        if (ok && used) {
            PixEval e;
            if (prob.eval_k(k, xf, ahf, e)) {                                  // (it does: F(xf) is finite)
                r[0] = e.r[0]; r[1] = e.r[1];
                Xn[0] = e.X[0]; Xn[1] = e.X[1]; Xn[2] = e.X[2];
                const double r2 = r[0] * r[0] + r[1] * r[1];
                if (c) s2 = s2 + r2; else s1 = s1 + r2;
                rmax = fmax(rmax, sqrt(r2));
            }
        }
        if (out.res) { out.res[at * 2] = r[0]; out.res[at * 2 + 1] = r[1]; }
        if (out.X) { out.X[at * 3] = Xn[0]; out.X[at * 3 + 1] = Xn[1]; out.X[at * 3 + 2] = Xn[2]; }
        if (out.pt_state) out.pt_state[at] = used ? 0 : (((gated >> i) & 1ull) ? 2 : 1);
    }
    for (int c = 0; c < 2; c++)
        for (int slot = (c ? n2 : n1) + lane; slot < MAXP; slot += 64) {
            const size_t at = ((size_t)f * 2 + c) * MAXP + slot;
            if (out.res) { out.res[at * 2] = 0; out.res[at * 2 + 1] = 0; }
            if (out.X) { out.X[at * 3] = 0; out.X[at * 3 + 1] = 0; out.X[at * 3 + 2] = 0; }
            if (out.pt_state) out.pt_state[at] = -1;
        }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
    if (lane == 0) {
        for (int a = 0; a < 6; a++) out.cyl[(size_t)f * 6 + a] = ok ? xf[a] : 0.0;
        out.fvals[2 * (size_t)f] = ok ? f0 : 0.0;
        out.fvals[2 * (size_t)f + 1] = ok ? ffinal : 0.0;
        out.iters[2 * (size_t)f] = ok ? itercount : 0;
        out.iters[2 * (size_t)f + 1] = ok ? func_evals : 0;
        int *oc = out.counts + 4 * (size_t)f;
        oc[0] = c1; oc[1] = c2; oc[2] = c_ref; oc[3] = c_gate;
        double *os = out.stats + 4 * (size_t)f;
        os[0] = ok && c1 > 0 ? sqrt(s1 / (double)c1) : 0.0;
        os[1] = ok && c2 > 0 ? sqrt(s2 / (double)c2) : 0.0;
        os[2] = ok ? sqrt(ffinal / (double)(c1 + c2)) : 0.0;
        os[3] = ok ? rmax : 0.0;
        out.status[f] = ok ? CPE_ST_OK : CPE_ST_FEW_POINTS;
    }
}

// ---- BUILD-DEFINED (include/cpe.h cpe_multi_frame_fit_pixels_batch, whose numbered rule this follows): T_Cam_AGV fitted to the
// pixels of every frame of a group at once.  The objective is PixFrame's, the pose step and the cross-wave sums are
// MultiPoseProblem's, the loop is lm_minimize<6>.
// k_multi_frame_pixels: one workgroup of MFPX_WAVES wavefronts per group.  Wave w takes kept frames w, w + WAVES, ... in order,
// lane l of it the detections l, l + 64, ... of a frame's concatenated list.  The table is staged in LDS once per workgroup.
// Membership of S: a group can hold 1024 frames of 4096 detections, so it does not fit registers; the store is the output
// pt_state itself.  The selection pass writes it, every later pass reads pt_state == 0.  With the fixed frame -> wave and slot ->
// lane assignment a lane only ever reads the words it wrote itself, so no fence and no barrier stands between the passes.  (The
// ranges of two groups of one call may therefore not share a frame.)
// F: every lane adds its members' squares in frame order then slot order; the 64-lane tree; the waves' sums are added in wave
// order; the NaN flag is an OR over the waves.  Both go through two alternating LDS rows, one barrier per evaluation, as
// MultiObjectiveT's terms do.  EVERY wave of the workgroup must make the same sequence of calls.
#ifndef CPE_MFPX_WAVES
#define CPE_MFPX_WAVES 4
#endif
constexpr int MFPX_WAVES = CPE_MFPX_WAVES;   // profiles/r33_resource_usage_multiframe_pixels.txt: 4 and 8 measured

struct MultiPixOut {
    double *x, *T, *fvals;
    int *iters, *nused, *counts;
    double *stats;
    int *status;
    double *N;                     // optional
    int *pt_state;
    double *frame_cyl, *frame_stats;
    double *res;                   // optional
    // a group that is not fitted: its status, every other per-group output zero
    __device__ void write_failed(int g, int st) const
    {
        if (threadIdx.x != 0) return;
        for (int k = 0; k < 6; k++) x[6 * (size_t)g + k] = 0;
        for (int k = 0; k < 16; k++) T[16 * (size_t)g + k] = 0;
        for (int k = 0; k < 2; k++) { fvals[2 * (size_t)g + k] = 0; iters[2 * (size_t)g + k] = 0; }
        for (int k = 0; k < 4; k++) { counts[4 * (size_t)g + k] = 0; stats[4 * (size_t)g + k] = 0; }
        if (N)
            for (int k = 0; k < 21; k++) N[21 * (size_t)g + k] = 0;
        nused[g] = 0;
        status[g] = st;
    }
};

template <int WAVES>
struct MultiPixProblem {
    PixFrame fr;                   // the table, the cameras and the gates; the frame's tables are set by frame()
    const double *xy1, *xy2;       // the call's tables (nullptr: the camera is absent)
    const int *id1, *id2, *cnt1, *cnt2;
    const double *TAGV;
    const int *pt_state;
    const int *sIdx;               // LDS, kept frames in order
    double *sJ;                    // LDS, [WAVES][MFLM_SUMS]
    double *sF;                    // LDS, [2][WAVES]
    int *sBad;                     // LDS, [2][WAVES]
    int nk, wave, lane, row;
    double T[16];                  // the pose normal() was last called at

    __device__ __forceinline__ void frame(int f)
    {
        const size_t tb = (size_t)f * MAXP * 2;
        fr.xy1 = xy1 ? xy1 + tb : nullptr; fr.xy2 = xy2 ? xy2 + tb : nullptr;
        fr.id1 = id1 ? id1 + tb : nullptr; fr.id2 = id2 ? id2 + tb : nullptr;
        const int n1 = xy1 ? min(max(cnt1[f], 0), MAXP) : 0, n2 = xy2 ? min(max(cnt2[f], 0), MAXP) : 0;
        fr.n1 = n1; fr.n12 = n1 + n2;
    }
    // the word of pt_state that stands for detection k of the frame's concatenated list
    __device__ __forceinline__ size_t slot_of(int f, int k) const
    {
        const int c = k >= fr.n1;
        return ((size_t)f * 2 + c) * MAXP + (c ? k - fr.n1 : k);
    }
    // rule 2: (o, a) of frame f at the pose Tm -> usable; ah = a / |a|
    __device__ __forceinline__ bool frame_pose(const double *Tm, int f, double *oa, double *ah, double &an) const
    {
        frame_axis(Tm, TAGV + 16 * (size_t)f, oa, oa + 3);
        return PixFrame::pose(oa, ah, an);
    }
    // rule 4
    __device__ __forceinline__ double operator()(const double *x)
    {
        double Tm[16], acc = 0.0;
        pose_vec2T(x, Tm);
        bool bad = false;
#pragma unroll
        for (int a = 0; a < 6; a++) bad = bad || !isfinite(x[a]);
        for (int kf = wave; kf < nk; kf += WAVES) {
            const int f = sIdx[kf];
            double oa[6], ah[3], an;
            frame(f);
            if (!frame_pose(Tm, f, oa, ah, an)) bad = true;
            for (int k = lane; k < fr.n12; k += 64) {
                if (pt_state[slot_of(f, k)] != 0) continue;
                PixEval e;
                if (!fr.eval_k(k, oa, ah, e)) { bad = true; continue; }
                acc = acc + (e.r[0] * e.r[0] + e.r[1] * e.r[1]);
            }
        }
        acc = wave_sum(acc);
        const int wbad = __ballot(bad) != 0ull;
        double *rf = sF + row * WAVES;
        int *rb = sBad + row * WAVES;
        row ^= 1;
        if (lane == 0) { rf[wave] = acc; rb[wave] = wbad; }
        __syncthreads();
        double v = 0.0;
        int any = 0;
        for (int w = 0; w < WAVES; w++) { v = v + rf[w]; any |= rb[w]; }
        return any ? __longlong_as_double(0x7ff8000000000000ll) : v;
    }
    // rule 6
    __device__ __forceinline__ void normal(const double *x, double *A, double *g)
    {
        pose_vec2T(x, T);
        double acc[MFLM_SUMS];
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) acc[k] = 0.0;
        for (int kf = wave; kf < nk; kf += WAVES) {
            const int f = sIdx[kf];
            const double *Am = TAGV + 16 * (size_t)f;
            double oa[6], ah[3], an, q[3];
            frame(f);
            frame_pose(T, f, oa, ah, an);
#pragma unroll
            for (int r = 0; r < 3; r++) q[r] = (T[r * 4] * Am[3] + T[r * 4 + 1] * Am[7]) + T[r * 4 + 2] * Am[11];
            for (int k = lane; k < fr.n12; k += 64) {
                if (pt_state[slot_of(f, k)] != 0) continue;
                PixEval e;
                if (!fr.eval_k(k, oa, ah, e)) continue;
                double dt[6], sx, sy, mu[3], aw[3];
                fr.node_derivatives(e, oa, ah, an, dt, sx, sy);
                cross3(q, dt, mu);
                cross3(oa + 3, dt + 3, aw);
                const double jp[6] = {mu[0] + aw[0], mu[1] + aw[1], mu[2] + aw[2], dt[0], dt[1], dt[2]};
                double j[6];
#pragma unroll
                for (int a = 0; a < 6; a++) j[a] = sx * jp[a];
                normal_accumulate<6>(j, e.r[0], acc);
#pragma unroll
                for (int a = 0; a < 6; a++) j[a] = sy * jp[a];
                normal_accumulate<6>(j, e.r[1], acc);
            }
        }
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) {
            const double s = wave_sum(acc[k]);
            if (lane == 0) sJ[wave * MFLM_SUMS + k] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) {
            double s = 0.0;
            for (int w = 0; w < WAVES; w++) s = s + sJ[w * MFLM_SUMS + k];
            if (k < 21) A[k] = s;
            else g[k - 21] = s;
        }
    }
    // the left perturbation of MultiPoseProblem::candidate
    __device__ __forceinline__ bool candidate(const double *, const double *dl, double *xn) const
    {
        double E[9], Tn[16];
        rot_exp(dl, E);
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) Tn[r * 4 + c] = (E[r * 3] * T[c] + E[r * 3 + 1] * T[4 + c]) + E[r * 3 + 2] * T[8 + c];
            Tn[r * 4 + 3] = T[r * 4 + 3] + dl[3 + r];
        }
        Tn[12] = 0; Tn[13] = 0; Tn[14] = 0; Tn[15] = 1;
        pose_T2vec(Tn, xn);
        return true;
    }
};

constexpr int MFPX_CNT = 5;      // |S| of camera 1 | of camera 2 | refused | gated | kept frames with a member
constexpr int MFPX_ST = 3;       // the squares of camera 1 | of camera 2 | the largest residual norm

// Barriers: multi_group_begin's, one after the selection's counts, one per objective evaluation and per Jacobian pass, two
// around the closing sums.  None stands under a condition that depends on the wave or the lane; every branch that holds one
// is taken on numbers that all waves have alike (LDS sums, the group's inputs).
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_multi_frame_pixels(
    const double *__restrict__ xy1, const int *__restrict__ id1, const int *__restrict__ cnt1, const double *__restrict__ xy2,
    const int *__restrict__ id2, const int *__restrict__ cnt2, const double *__restrict__ TAGV, const int *__restrict__ frame_ok,
    const int *__restrict__ group_start, int n, const double *__restrict__ x0_in, double R, const double *__restrict__ K1,
    const double *__restrict__ K2, const double *__restrict__ T21, const double *__restrict__ P,
    const int *__restrict__ line_status, int lo, int L, const double *__restrict__ centre, int swap, double min_cos, double sel_cos,
    double gate_px, double tolx, double tolf, int maxiter, const MultiPixOut out)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ double sP[2 * CPE_MAXL * 4];
    __shared__ int sSt[2 * CPE_MAXL];
    __shared__ int sIdx[MF_MAXF];
    __shared__ double sJ[WAVES * MFLM_SUMS];
    __shared__ double sF[2 * WAVES];
    __shared__ int sBad[2 * WAVES];
    __shared__ int sCnt[WAVES * MFPX_CNT];
    __shared__ double sSt3[WAVES * MFPX_ST];
    __shared__ int sNk;
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 8 * L; i += 64 * WAVES) sP[i] = P[i];
    for (int i = threadIdx.x; i < 2 * L; i += 64 * WAVES) sSt[i] = line_status[i];
    const int nk = multi_group_begin(frame_ok, group_start, n, g, sIdx, &sNk, out);   // (its barrier covers the staging)
    const int ga = group_start[g], gb = group_start[g + 1];
    const bool range_ok = 0 <= ga && ga <= gb && gb <= n;

    // rule 1
    double x0[6] = {0, 0, 0, 0, 0, 0};
    bool run = nk != 0;
    if (run) {
#pragma unroll
        for (int a = 0; a < 6; a++) { x0[a] = x0_in[6 * (size_t)g + a]; run = run && isfinite(x0[a]); }
        if (!run) out.write_failed(g, CPE_ST_FEW_POINTS);
    }
    // pt_state of every frame of the range: -1 past the counts, 1 below them except where the selection is going to decide
    if (range_ok)
        for (int f = ga + wave; f < gb; f += WAVES) {
            const bool sel = run && (frame_ok == nullptr || frame_ok[f] != 0);
            for (int c = 0; c < 2; c++) {
                const int *cn = c ? cnt2 : cnt1;
                const int m = (c ? xy2 : xy1) ? min(max(cn[f], 0), MAXP) : 0;
                int *ps = out.pt_state + ((size_t)f * 2 + c) * MAXP;
                for (int s = sel ? m + lane : lane; s < MAXP; s += 64) ps[s] = s < m ? 1 : -1;
            }
        }
    if (!run) return;

    MultiPixProblem<WAVES> prob;
    prob.fr.sP = sP; prob.fr.sSt = sSt;
    prob.fr.lo = lo; prob.fr.hi = lo + (L - 1); prob.fr.L = L; prob.fr.swap = swap;
    prob.fr.R = R; prob.fr.min_cos = sel_cos;
#pragma unroll
    for (int a = 0; a < 3; a++) { prob.fr.centre[a] = centre[a]; prob.fr.t2[a] = T21[4 * a + 3]; }
    tri_cam(K1, nullptr, prob.fr.cam1);
    tri_cam(K2, T21, prob.fr.cam2);
    prob.fr.lane = lane;
    prob.xy1 = xy1; prob.xy2 = xy2; prob.id1 = id1; prob.id2 = id2; prob.cnt1 = cnt1; prob.cnt2 = cnt2;
    prob.TAGV = TAGV; prob.pt_state = out.pt_state; prob.sIdx = sIdx; prob.sJ = sJ; prob.sF = sF; prob.sBad = sBad;
    prob.nk = nk; prob.wave = wave; prob.lane = lane; prob.row = 0;

    // rule 3: the used set, once, at x0 with sel_cos
    {
        double T0[16];
        pose_vec2T(x0, T0);
        int cs[MFPX_CNT] = {0, 0, 0, 0, 0};
        for (int kf = wave; kf < nk; kf += WAVES) {
            const int f = sIdx[kf];
            double oa[6], ah[3], an;
            prob.frame(f);
            const bool pose_ok = prob.frame_pose(T0, f, oa, ah, an);
            int members = 0;
            for (int k = lane; k < prob.fr.n12; k += 64) {
                PixEval e;
                int st = 1;
                if (pose_ok && prob.fr.eval_k(k, oa, ah, e)) {
                    const double r2 = e.r[0] * e.r[0] + e.r[1] * e.r[1];
                    st = (gate_px > 0 && sqrt(r2) >= gate_px) ? 2 : 0;
                }
                out.pt_state[prob.slot_of(f, k)] = st;
                cs[0] += st == 0 && k < prob.fr.n1; cs[1] += st == 0 && k >= prob.fr.n1; cs[2] += st == 1; cs[3] += st == 2;
                members += st == 0;
            }
            cs[4] += __ballot(members != 0) != 0ull;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) cs[k] = wave_sum_i(cs[k]);
        if (lane == 0)
            for (int k = 0; k < MFPX_CNT; k++) sCnt[wave * MFPX_CNT + k] = cs[k];
    }
    __syncthreads();
    int cs[MFPX_CNT] = {0, 0, 0, 0, 0};
    for (int w = 0; w < WAVES; w++)
        for (int k = 0; k < MFPX_CNT; k++) cs[k] += sCnt[w * MFPX_CNT + k];
    const int nS = cs[0] + cs[1];
    if (nS < CPE_PIXFIT_MIN_PTS || cs[4] < 2) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }

    // rules 4, 5
    prob.fr.min_cos = min_cos;
    const double f0 = prob(x0);
    if (!fit_finite(x0, f0)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    double x[6], fx;
    int itercount, func_evals = 1;
    lm_minimize<6>(prob, x0, f0, tolx, tolf, maxiter, x, fx, itercount, func_evals);
    if (!fit_finite(x, fx)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }

    // rule 7: the per-frame outputs and the group's statistics at x
    double Tf[16];
    pose_vec2T(x, Tf);
    double gs[MFPX_ST] = {0, 0, 0};
    for (int kf = wave; kf < nk; kf += WAVES) {
        const int f = sIdx[kf];
        double oa[6], ah[3], an, s1 = 0.0, s2 = 0.0, rmax = 0.0;
        int m1 = 0, m2 = 0;
        prob.frame(f);
        prob.frame_pose(Tf, f, oa, ah, an);
        const int n1 = prob.fr.n1, n12 = prob.fr.n12;
        for (int k = lane; k < n12; k += 64) {
            const size_t at = prob.slot_of(f, k);
            double r[2] = {0, 0};
            if (out.pt_state[at] == 0) {
                PixEval e;
                if (prob.fr.eval_k(k, oa, ah, e)) {                                // (it does: F(x) is finite)
                    r[0] = e.r[0]; r[1] = e.r[1];
                    const double r2 = r[0] * r[0] + r[1] * r[1];
                    if (k >= n1) { s2 = s2 + r2; m2++; } else { s1 = s1 + r2; m1++; }
                    rmax = fmax(rmax, sqrt(r2));
                }
            }
            if (out.res) { out.res[at * 2] = r[0]; out.res[at * 2 + 1] = r[1]; }
        }
        if (out.res)
            for (int c = 0; c < 2; c++)
                for (int s = (c ? n12 - n1 : n1) + lane; s < MAXP; s += 64) {
                    const size_t at = ((size_t)f * 2 + c) * MAXP + s;
                    out.res[at * 2] = 0; out.res[at * 2 + 1] = 0;
                }
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        m1 = wave_sum_i(m1); m2 = wave_sum_i(m2);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
        gs[0] = gs[0] + s1; gs[1] = gs[1] + s2; gs[2] = fmax(gs[2], rmax);
        if (lane == 0) {
            for (int a = 0; a < 6; a++) out.frame_cyl[6 * (size_t)f + a] = oa[a];
            double *fs = out.frame_stats + 4 * (size_t)f;
            fs[0] = m1 > 0 ? sqrt(s1 / (double)m1) : 0.0;
            fs[1] = m2 > 0 ? sqrt(s2 / (double)m2) : 0.0;
            fs[2] = m1 + m2 > 0 ? sqrt((s1 + s2) / (double)(m1 + m2)) : 0.0;
            fs[3] = rmax;
        }
    }
    __syncthreads();                                   // every wave has read the sums of the loop's last Jacobian pass
    if (lane == 0)
        for (int k = 0; k < MFPX_ST; k++) sSt3[wave * MFPX_ST + k] = gs[k];
    double A[21], gr[6];
    if (out.N) prob.normal(x, A, gr);                  // (one barrier; out.N is the same for every wave)
    else __syncthreads();
    if (threadIdx.x == 0) {
        double S1 = 0.0, S2 = 0.0, rmax = 0.0;
        for (int w = 0; w < WAVES; w++) {
            S1 = S1 + sSt3[w * MFPX_ST]; S2 = S2 + sSt3[w * MFPX_ST + 1]; rmax = fmax(rmax, sSt3[w * MFPX_ST + 2]);
        }
        for (int k = 0; k < 6; k++) out.x[6 * (size_t)g + k] = x[k];
        for (int k = 0; k < 16; k++) out.T[16 * (size_t)g + k] = Tf[k];
        out.fvals[2 * (size_t)g] = f0; out.fvals[2 * (size_t)g + 1] = fx;
        out.iters[2 * (size_t)g] = itercount; out.iters[2 * (size_t)g + 1] = func_evals;
        out.nused[g] = nk;
        for (int k = 0; k < 4; k++) out.counts[4 * (size_t)g + k] = cs[k];
        double *os = out.stats + 4 * (size_t)g;
        os[0] = cs[0] > 0 ? sqrt(S1 / (double)cs[0]) : 0.0;
        os[1] = cs[1] > 0 ? sqrt(S2 / (double)cs[1]) : 0.0;
        os[2] = sqrt(fx / (double)nS);
        os[3] = rmax;
        if (out.N)
            for (int k = 0; k < 21; k++) out.N[21 * (size_t)g + k] = A[k];
        out.status[g] = CPE_ST_OK;
    }
}

// ---- BUILD-DEFINED (include/cpe.h cpe_multi_frame_fit_pixels_angles_batch, whose numbered rule this follows): T_Cam_AGV and the
// (pan, tilt) of every kept frame fitted jointly to the pixels of a group, the angles held at their nominal values by a prior.
// The system is an arrowhead: 6 shared unknowns x, 2 per kept frame q_i, and q_i meets only frame i's rows.
// k_multi_frame_pixels_angles: k_multi_frame_pixels' layout (wave w takes kept frames w, w + WAVES, ...; lane l the detections l,
// l + 64, ...; the table in LDS; membership of S in pt_state), its problem reused for the tables, the pose step and the LDS rows.
// New is the per-frame state in LDS, MFJ_FRAME doubles per kept frame: the two angle pairs (the current one and the trial, which
// swap roles on an accepted trial, so nothing is copied) and the frame's blocks V_i, W_i, g_i.  Only the wave that owns a frame
// ever touches its state: lane 0 writes the blocks at the end of the frame in the Jacobian pass, and in the trial solve lane j of
// wave w takes the wave's j-th frame.  So the barriers of the passes are all the ordering the state needs.
constexpr int MFJ_MAXF = CPE_MFJOINT_MAXF;
constexpr int MFJ_WAVES = 4;                                        // the LDS below is sized for it: 63.9 KB of the 64 KB
constexpr int MFJ_V = 4, MFJ_W = 7, MFJ_G = 19, MFJ_FRAME = 21;   // q[2][2] | V 00 01 11 | W[6][2] | g[2]
constexpr int MFJ_LOCAL = 17;                                       // the sums of a frame's blocks: V | W | g
constexpr int MFJ_RED = MFLM_SUMS + 1;                              // sum Y W' (21) | sum Y g (6) | a singular V_i
constexpr double MFJ_TILT_MAX = 1.5707963267948966 - 1e-3;         // k_frame_angles_lm's: tan(tilt) of the chain has its pole at pi/2

struct MultiJointOut : MultiPixOut {
    double *angles;
    double *frame_N;               // optional
};

template <int WAVES>
struct MultiJointProblem : MultiPixProblem<WAVES> {
    using Base = MultiPixProblem<WAVES>;
    const double *angles0;
    double *sFr;                   // LDS, [nk][MFJ_FRAME]
    double *sRed;                  // LDS, [2][WAVES][MFJ_RED]
    double *sD;                    // LDS, [2][WAVES]: the waves' largest |dq| of the trial being evaluated
    double wp2, wt2;               // the prior weights, squared
    int cur, rrow;                 // the angle pair that is the current point; the row of sRed to write next
    double dq_wave, dq_max;        // the largest |dq| of this wave's frames; of all (after operator())

    __device__ __forceinline__ double *state(int kf) const { return sFr + kf * MFJ_FRAME; }
    // rule 2: the chain, (o, a) and ah = a / |a| of a frame with the angles q at the pose Tm -> usable
    __device__ __forceinline__ static bool frame_pose_at(const double *Tm, const double *q, double *A, double *oa, double *ah, double &an)
    {
        agv_chain(q[0], q[1], A);
        frame_axis(Tm, A, oa, oa + 3);
        return PixFrame::pose(oa, ah, an) && isfinite(q[0]) && isfinite(q[1]) && fabs(q[1]) < MFJ_TILT_MAX;
    }
    // rule 4 at (x, the angle pairs `sel`)
    __device__ __forceinline__ double evaluate(const double *x, int sel)
    {
        double Tm[16], acc = 0.0;
        pose_vec2T(x, Tm);
        bool bad = false;
#pragma unroll
        for (int a = 0; a < 6; a++) bad = bad || !isfinite(x[a]);
        for (int kf = this->wave; kf < this->nk; kf += WAVES) {
            const int f = this->sIdx[kf];
            const double q[2] = {state(kf)[2 * sel], state(kf)[2 * sel + 1]};
            double A[16], oa[6], ah[3], an;
            this->frame(f);
            if (!frame_pose_at(Tm, q, A, oa, ah, an)) bad = true;
            for (int k = this->lane; k < this->fr.n12; k += 64) {
                if (this->pt_state[this->slot_of(f, k)] != 0) continue;
                PixEval e;
                if (!this->fr.eval_k(k, oa, ah, e)) { bad = true; continue; }
                acc = acc + (e.r[0] * e.r[0] + e.r[1] * e.r[1]);
            }
            if (this->lane == 0) {
                const double d0 = q[0] - angles0[2 * (size_t)f], d1 = q[1] - angles0[2 * (size_t)f + 1];
                acc = acc + (wp2 * (d0 * d0) + wt2 * (d1 * d1));
            }
        }
        acc = wave_sum(acc);
        const int wbad = __ballot(bad) != 0ull;
        double *rf = this->sF + this->row * WAVES, *rd = sD + this->row * WAVES;
        int *rb = this->sBad + this->row * WAVES;
        this->row ^= 1;
        if (this->lane == 0) { rf[this->wave] = acc; rb[this->wave] = wbad; rd[this->wave] = dq_wave; }
        __syncthreads();
        double v = 0.0;
        int any = 0;
        dq_max = 0.0;
        for (int w = 0; w < WAVES; w++) { v = v + rf[w]; any |= rb[w]; dq_max = fmax(dq_max, rd[w]); }
        return any ? __longlong_as_double(0x7ff8000000000000ll) : v;
    }
    __device__ __forceinline__ double operator()(const double *xn) { return evaluate(xn, cur ^ 1); }   // the trial
    __device__ __forceinline__ void accept() { cur ^= 1; }

    // rule 6 at (x, the current angles): U and g_x to every wave, the frames' blocks into their states.  One sweep over this
    // wave's frames with all 44 accumulators: the 27 sums of the pose columns, and each frame's 17, reduced at the end of the
    // frame, the prior added.  No scratch: profiles/r34_resource_usage_multiframe_joint.txt.  (Split in two sweeps, the 27 and
    // then the 17, it needs none either and makes every node twice: 27 - 34 % slower)
    __device__ __forceinline__ void normal(const double *x, double *U, double *gx)
    {
        pose_vec2T(x, this->T);
        const double *T = this->T;
        double acc[MFLM_SUMS];
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) acc[k] = 0.0;
        for (int kf = this->wave; kf < this->nk; kf += WAVES) {
            const int f = this->sIdx[kf];
            const double q[2] = {state(kf)[2 * cur], state(kf)[2 * cur + 1]};
            double A[16], oa[6], ah[3], an, m[3], da[6], dp[6], dob[6], dvb[6], loc[MFJ_LOCAL];
            this->frame(f);
            frame_pose_at(T, q, A, oa, ah, an);
#pragma unroll
            for (int r = 0; r < 3; r++) m[r] = (T[r * 4] * A[3] + T[r * 4 + 1] * A[7]) + T[r * 4 + 2] * A[11];
            agv_chain_derivatives(q[0], q[1], da, dp);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    dob[3 * j + r] = (T[r * 4] * dp[3 * j] + T[r * 4 + 1] * dp[3 * j + 1]) + T[r * 4 + 2] * dp[3 * j + 2];
                    dvb[3 * j + r] = (T[r * 4] * da[3 * j] + T[r * 4 + 1] * da[3 * j + 1]) + T[r * 4 + 2] * da[3 * j + 2];
                }
#pragma unroll
            for (int k = 0; k < MFJ_LOCAL; k++) loc[k] = 0.0;
            for (int k = this->lane; k < this->fr.n12; k += 64) {
                if (this->pt_state[this->slot_of(f, k)] != 0) continue;
                PixEval e;
                if (!this->fr.eval_k(k, oa, ah, e)) continue;
                double dt[6], s[2], mu[3], aw[3], jq[2];
                this->fr.node_derivatives(e, oa, ah, an, dt, s[0], s[1]);
                cross3(m, dt, mu);
                cross3(oa + 3, dt + 3, aw);
                const double jp[6] = {mu[0] + aw[0], mu[1] + aw[1], mu[2] + aw[2], dt[0], dt[1], dt[2]};
#pragma unroll
                for (int j = 0; j < 2; j++) jq[j] = dot3(dt, dob + 3 * j) + dot3(dt + 3, dvb + 3 * j);
#pragma unroll
                for (int c = 0; c < 2; c++) {                              // the x row, then the y row
                    double j[6];
#pragma unroll
                    for (int a = 0; a < 6; a++) j[a] = s[c] * jp[a];
                    normal_accumulate<6>(j, e.r[c], acc);
                    const double j6 = s[c] * jq[0], j7 = s[c] * jq[1];
                    loc[0] = loc[0] + j6 * j6; loc[1] = loc[1] + j6 * j7; loc[2] = loc[2] + j7 * j7;
#pragma unroll
                    for (int a = 0; a < 6; a++) {
                        loc[3 + 2 * a] = loc[3 + 2 * a] + j[a] * j6;
                        loc[4 + 2 * a] = loc[4 + 2 * a] + j[a] * j7;
                    }
                    loc[15] = loc[15] + j6 * e.r[c]; loc[16] = loc[16] + j7 * e.r[c];
                }
            }
            double *st = state(kf);
            const double d0 = q[0] - angles0[2 * (size_t)f], d1 = q[1] - angles0[2 * (size_t)f + 1];
#pragma unroll
            for (int k = 0; k < MFJ_LOCAL; k++) {
                double v = wave_sum(loc[k]);
                if (k == 0) v = v + wp2;
                if (k == 2) v = v + wt2;
                if (k == 15) v = v + wp2 * d0;
                if (k == 16) v = v + wt2 * d1;
                if (this->lane == 0) st[MFJ_V + k] = v;
            }
        }
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) {
            const double s = wave_sum(acc[k]);
            if (this->lane == 0) this->sJ[this->wave * MFLM_SUMS + k] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) {
            double s = 0.0;
            for (int w = 0; w < WAVES; w++) s = s + this->sJ[w * MFLM_SUMS + k];
            if (k < 21) U[k] = s;
            else gx[k - 21] = s;
        }
    }
    // the 2 x 2 block of a frame as rule 7 damps it (DAMPED) or as it stands -> its determinant
    template <bool DAMPED>
    __device__ __forceinline__ static double block(const double *st, double lambda, double &m00, double &m11)
    {
        const double v0 = st[MFJ_V], v1 = st[MFJ_V + 1], v2 = st[MFJ_V + 2], tr = v0 + v2;
        m00 = DAMPED ? v0 + lambda * v0 + 1e-12 * tr : v0;
        m11 = DAMPED ? v2 + lambda * v2 + 1e-12 * tr : v2;
        return m00 * m11 - v1 * v1;
    }
    // rule 7's sums over ALL kept frames: R[0..20] = sum Y_i W_i' (upper triangle), R[21..26] = sum Y_i g_i.  Every wave adds its
    // own frames (lane j its j-th), the waves are added in wave order: all waves hold the same numbers.  -> no block was singular
    template <bool DAMPED>
    __device__ __forceinline__ bool reduce(double lambda, double *R)
    {
        double acc[MFLM_SUMS];
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) acc[k] = 0.0;
        bool sing = false;
        for (int kf = this->wave + WAVES * this->lane; kf < this->nk; kf += WAVES * 64) {
            const double *st = state(kf), *W = st + MFJ_W, *g = st + MFJ_G;
            double m00, m11, Y[12];
            const double det = block<DAMPED>(st, lambda, m00, m11), v1 = st[MFJ_V + 1];
            sing = sing || det == 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                Y[2 * a] = (W[2 * a] * m11 - W[2 * a + 1] * v1) / det;
                Y[2 * a + 1] = (W[2 * a + 1] * m00 - W[2 * a] * v1) / det;
            }
            int i = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int b = a; b < 6; b++) { acc[i] = acc[i] + (Y[2 * a] * W[2 * b] + Y[2 * a + 1] * W[2 * b + 1]); i++; }
                acc[21 + a] = acc[21 + a] + (Y[2 * a] * g[0] + Y[2 * a + 1] * g[1]);
            }
        }
        double *rr = sRed + (rrow * WAVES + this->wave) * MFJ_RED;
        const double *all = sRed + rrow * WAVES * MFJ_RED;
        rrow ^= 1;
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) {
            const double s = wave_sum(acc[k]);
            if (this->lane == 0) rr[k] = s;
        }
        const bool wsing = __ballot(sing) != 0ull;
        if (this->lane == 0) rr[MFLM_SUMS] = wsing ? 1.0 : 0.0;
        __syncthreads();
        bool any = false;
#pragma unroll
        for (int k = 0; k < MFLM_SUMS; k++) R[k] = 0.0;
        for (int w = 0; w < WAVES; w++) {
#pragma unroll
            for (int k = 0; k < MFLM_SUMS; k++) R[k] = R[k] + all[w * MFJ_RED + k];
            any = any || all[w * MFJ_RED + MFLM_SUMS] != 0.0;
        }
        return !any;
    }
    // rule 7: one damped trial from (x, the current angles) -> dx, the candidate xn, and the trial angles in the frames' states;
    // false: a block was singular, nothing may be evaluated.  (Two barriers when it succeeds, one when the 6 x 6 system fails,
    // the same for every wave: the numbers they branch on are the same.)
    __device__ __forceinline__ bool trial(const double *U, const double *gx, double lambda, double *dx, double *xn)
    {
        double R[MFLM_SUMS], M[36], rhs[6];
        const bool blocks_ok = reduce<true>(lambda, R);
        int i = 0;
        double trU = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) { if (a == b) trU = trU + U[i]; i++; }
        i = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int b = a; b < 6; b++) {
                const double u = a == b ? U[i] + lambda * U[i] + 1e-12 * trU : U[i];
                M[a * 6 + b] = u - R[i];
                M[b * 6 + a] = u - R[i];
                i++;
            }
            rhs[a] = -gx[a] + R[21 + a];
        }
        if (!gauss_solve<6>(M, rhs, dx) || !blocks_ok) return false;
        double dmax = 0.0;
        for (int kf = this->wave + WAVES * this->lane; kf < this->nk; kf += WAVES * 64) {
            double *st = state(kf);
            const double *W = st + MFJ_W;
            double m00, m11, t0 = st[MFJ_G], t1 = st[MFJ_G + 1];
            const double det = block<true>(st, lambda, m00, m11), v1 = st[MFJ_V + 1];
#pragma unroll
            for (int a = 0; a < 6; a++) { t0 = t0 + W[2 * a] * dx[a]; t1 = t1 + W[2 * a + 1] * dx[a]; }
            const double d0 = (v1 * t1 - m11 * t0) / det, d1 = (v1 * t0 - m00 * t1) / det;   // lm_damped_solve<2>'s form
            // (a zero step keeps the angle's bits, rule 9: -0.0 + 0.0 would be +0.0)
            st[2 * (cur ^ 1)] = d0 == 0.0 ? st[2 * cur] : st[2 * cur] + d0;
            st[2 * (cur ^ 1) + 1] = d1 == 0.0 ? st[2 * cur + 1] : st[2 * cur + 1] + d1;
            dmax = fmax(dmax, fmax(fabs(d0), fabs(d1)));
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off, 64));
        dq_wave = dmax;
        __syncthreads();                               // the trial angles, written per lane, are read per frame by the whole wave
        return this->candidate(nullptr, dx, xn);
    }
};

// Levenberg-Marquardt on an arrowhead system (shared unknowns x, per-block unknowns that the problem keeps itself): the sibling
// of lm_minimize, with its rules, for a problem that eliminates its blocks.  A problem supplies
//   normal(x, U, g)                  one Jacobian pass at the current point: the shared block (packed) and gradient
//   bool trial(U, g, lambda, dx, xn) the damped block solve, the step dx and the candidate xn (its block unknowns inside the
//                                    problem); false: singular, xn may not be evaluated
//   double operator()(xn)            the objective at the candidate; dq_max: the largest block step of it
//   accept()                         the candidate's block unknowns become the current ones
// The constants are lm_minimize's and stand here once.  Barriers: as lm_minimize says, no branch may depend on the wave or lane.
template <int N, class Problem>
__device__ __forceinline__ void lm_minimize_arrowhead(Problem &prob, const double *x0, double f0, double tolx, double tolf, int maxiter,
                                                      double *x, double &fx, int &itercount, int &func_evals)
{
    constexpr double LAMBDA0 = 1e-3, LAMBDA_STEP = 10, LAMBDA_MIN = 1e-12, TOLF_SCALE = 1e-3;
    constexpr int TRIALS = 12, MAX_ITER = 200;
#pragma unroll
    for (int k = 0; k < N; k++) x[k] = x0[k];
    fx = f0;
    double lambda = LAMBDA0;
    itercount = 0;
    for (; itercount < maxiter && itercount < MAX_ITER;) {
        double U[N * (N + 1) / 2], g[N];
        prob.normal(x, U, g);
        itercount++;
        bool accepted = false;
        double dmax = 0;
        const double fprev = fx;
        for (int tr = 0; tr < TRIALS && !accepted; tr++) {
            double dx[N], xn[N];
            if (!prob.trial(U, g, lambda, dx, xn)) { lambda = lambda * LAMBDA_STEP; continue; }
            const double fn = prob(xn);
            func_evals++;
            if (fn < fx) {
                dmax = prob.dq_max;
#pragma unroll
                for (int k = 0; k < N; k++) dmax = fmax(dmax, fabs(dx[k]));
#pragma unroll
                for (int k = 0; k < N; k++) x[k] = xn[k];
                prob.accept();
                fx = fn;
                lambda = fmax(lambda / LAMBDA_STEP, LAMBDA_MIN);
                accepted = true;
            } else {
                lambda = lambda * LAMBDA_STEP;
            }
        }
        if (!accepted) break;
        if ((fprev - fx) <= tolf * TOLF_SCALE * (1.0 + fx) && dmax <= tolx) break;
    }
}

// Barriers: those of k_multi_frame_pixels, and two per trial solve (MultiJointProblem::trial).  None stands under a condition
// that depends on the wave or the lane.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_multi_frame_pixels_angles(
    const double *__restrict__ xy1, const int *__restrict__ id1, const int *__restrict__ cnt1, const double *__restrict__ xy2,
    const int *__restrict__ id2, const int *__restrict__ cnt2, const double *__restrict__ angles0, const int *__restrict__ frame_ok,
    const int *__restrict__ group_start, int n, const double *__restrict__ x0_in, double w_pan, double w_tilt, double R,
    const double *__restrict__ K1, const double *__restrict__ K2, const double *__restrict__ T21, const double *__restrict__ P,
    const int *__restrict__ line_status, int lo, int L, const double *__restrict__ centre, int swap, double min_cos, double sel_cos,
    double gate_px, double tolx, double tolf, int maxiter, const MultiJointOut out)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ double sP[2 * CPE_MAXL * 4];
    __shared__ int sSt[2 * CPE_MAXL];
    __shared__ int sIdx[MFJ_MAXF];
    __shared__ double sFr[MFJ_MAXF * MFJ_FRAME];
    __shared__ double sJ[WAVES * MFLM_SUMS];
    __shared__ double sRed[2 * WAVES * MFJ_RED];
    __shared__ double sF[2 * WAVES];
    __shared__ double sD[2 * WAVES];
    __shared__ int sBad[2 * WAVES];
    __shared__ int sCnt[WAVES * MFPX_CNT];
    __shared__ double sSt3[WAVES * MFPX_ST];
    __shared__ int sNk;
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 8 * L; i += 64 * WAVES) sP[i] = P[i];
    for (int i = threadIdx.x; i < 2 * L; i += 64 * WAVES) sSt[i] = line_status[i];
    const int nk = multi_group_begin<MFJ_MAXF>(frame_ok, group_start, n, g, sIdx, &sNk, out);   // (its barrier covers the staging)
    const int ga = group_start[g], gb = group_start[g + 1];
    const bool range_ok = 0 <= ga && ga <= gb && gb <= n;

    // rule 1
    double x0[6] = {0, 0, 0, 0, 0, 0};
    bool run = nk != 0;
    if (run) {
#pragma unroll
        for (int a = 0; a < 6; a++) { x0[a] = x0_in[6 * (size_t)g + a]; run = run && isfinite(x0[a]); }
        if (!run) out.write_failed(g, CPE_ST_FEW_POINTS);
    }
    // pt_state of every frame of the range: -1 past the counts, 1 below them except where the selection is going to decide
    if (range_ok)
        for (int f = ga + wave; f < gb; f += WAVES) {
            const bool sel = run && (frame_ok == nullptr || frame_ok[f] != 0);
            for (int c = 0; c < 2; c++) {
                const int *cn = c ? cnt2 : cnt1;
                const int m = (c ? xy2 : xy1) ? min(max(cn[f], 0), MAXP) : 0;
                int *ps = out.pt_state + ((size_t)f * 2 + c) * MAXP;
                for (int s = sel ? m + lane : lane; s < MAXP; s += 64) ps[s] = s < m ? 1 : -1;
            }
        }
    if (!run) return;

    MultiJointProblem<WAVES> prob;
    prob.fr.sP = sP; prob.fr.sSt = sSt;
    prob.fr.lo = lo; prob.fr.hi = lo + (L - 1); prob.fr.L = L; prob.fr.swap = swap;
    prob.fr.R = R; prob.fr.min_cos = sel_cos;
#pragma unroll
    for (int a = 0; a < 3; a++) { prob.fr.centre[a] = centre[a]; prob.fr.t2[a] = T21[4 * a + 3]; }
    tri_cam(K1, nullptr, prob.fr.cam1);
    tri_cam(K2, T21, prob.fr.cam2);
    prob.fr.lane = lane;
    prob.xy1 = xy1; prob.xy2 = xy2; prob.id1 = id1; prob.id2 = id2; prob.cnt1 = cnt1; prob.cnt2 = cnt2;
    prob.TAGV = nullptr; prob.pt_state = out.pt_state; prob.sIdx = sIdx; prob.sJ = sJ; prob.sF = sF; prob.sBad = sBad;
    prob.nk = nk; prob.wave = wave; prob.lane = lane; prob.row = 0;
    prob.angles0 = angles0; prob.sFr = sFr; prob.sRed = sRed; prob.sD = sD;
    prob.wp2 = w_pan * w_pan; prob.wt2 = w_tilt * w_tilt;
    prob.cur = 0; prob.rrow = 0; prob.dq_wave = 0.0; prob.dq_max = 0.0;

    // rule 3: the used set, once, at (x0, angles0) with sel_cos; the frames' states start at the nominal angles
    {
        double T0[16];
        pose_vec2T(x0, T0);
        int cs[MFPX_CNT] = {0, 0, 0, 0, 0};
        for (int kf = wave; kf < nk; kf += WAVES) {
            const int f = sIdx[kf];
            const double q[2] = {angles0[2 * (size_t)f], angles0[2 * (size_t)f + 1]};
            double A[16], oa[6], ah[3], an;
            prob.frame(f);
            const bool pose_ok = prob.frame_pose_at(T0, q, A, oa, ah, an);
            if (lane < MFJ_FRAME) prob.state(kf)[lane] = lane < 4 ? ((lane & 1) ? q[1] : q[0]) : 0.0;
            int members = 0;
            for (int k = lane; k < prob.fr.n12; k += 64) {
                PixEval e;
                int st = 1;
                if (pose_ok && prob.fr.eval_k(k, oa, ah, e)) {
                    const double r2 = e.r[0] * e.r[0] + e.r[1] * e.r[1];
                    st = (gate_px > 0 && sqrt(r2) >= gate_px) ? 2 : 0;
                }
                out.pt_state[prob.slot_of(f, k)] = st;
                cs[0] += st == 0 && k < prob.fr.n1; cs[1] += st == 0 && k >= prob.fr.n1; cs[2] += st == 1; cs[3] += st == 2;
                members += st == 0;
            }
            cs[4] += __ballot(members != 0) != 0ull;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) cs[k] = wave_sum_i(cs[k]);
        if (lane == 0)
            for (int k = 0; k < MFPX_CNT; k++) sCnt[wave * MFPX_CNT + k] = cs[k];
    }
    __syncthreads();
    int cs[MFPX_CNT] = {0, 0, 0, 0, 0};
    for (int w = 0; w < WAVES; w++)
        for (int k = 0; k < MFPX_CNT; k++) cs[k] += sCnt[w * MFPX_CNT + k];
    const int nS = cs[0] + cs[1];
    if (nS < CPE_PIXFIT_MIN_PTS || cs[4] < 2) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }

    // rules 4 to 8
    prob.fr.min_cos = min_cos;
    const double f0 = prob.evaluate(x0, prob.cur);
    if (!fit_finite(x0, f0)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }
    double x[6], fx;
    int itercount, func_evals = 1;
    lm_minimize_arrowhead<6>(prob, x0, f0, tolx, tolf, maxiter, x, fx, itercount, func_evals);
    if (!fit_finite(x, fx)) { out.write_failed(g, CPE_ST_FEW_POINTS); return; }

    // rule 10: the per-frame outputs and the group's statistics at (x, q)
    double Tf[16];
    pose_vec2T(x, Tf);
    double gs[MFPX_ST] = {0, 0, 0};
    for (int kf = wave; kf < nk; kf += WAVES) {
        const int f = sIdx[kf];
        const double q[2] = {prob.state(kf)[2 * prob.cur], prob.state(kf)[2 * prob.cur + 1]};
        double A[16], oa[6], ah[3], an, s1 = 0.0, s2 = 0.0, rmax = 0.0;
        int m1 = 0, m2 = 0;
        prob.frame(f);
        prob.frame_pose_at(Tf, q, A, oa, ah, an);
        const int n1 = prob.fr.n1, n12 = prob.fr.n12;
        for (int k = lane; k < n12; k += 64) {
            const size_t at = prob.slot_of(f, k);
            double r[2] = {0, 0};
            if (out.pt_state[at] == 0) {
                PixEval e;
                if (prob.fr.eval_k(k, oa, ah, e)) {                                // (it does: F(x, q) is finite)
                    r[0] = e.r[0]; r[1] = e.r[1];
                    const double r2 = r[0] * r[0] + r[1] * r[1];
                    if (k >= n1) { s2 = s2 + r2; m2++; } else { s1 = s1 + r2; m1++; }
                    rmax = fmax(rmax, sqrt(r2));
                }
            }
            if (out.res) { out.res[at * 2] = r[0]; out.res[at * 2 + 1] = r[1]; }
        }
        if (out.res)
            for (int c = 0; c < 2; c++)
                for (int s = (c ? n12 - n1 : n1) + lane; s < MAXP; s += 64) {
                    const size_t at = ((size_t)f * 2 + c) * MAXP + s;
                    out.res[at * 2] = 0; out.res[at * 2 + 1] = 0;
                }
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        m1 = wave_sum_i(m1); m2 = wave_sum_i(m2);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, off, 64));
        gs[0] = gs[0] + s1; gs[1] = gs[1] + s2; gs[2] = fmax(gs[2], rmax);
        if (lane == 0) {
            for (int a = 0; a < 6; a++) out.frame_cyl[6 * (size_t)f + a] = oa[a];
            out.angles[2 * (size_t)f] = q[0]; out.angles[2 * (size_t)f + 1] = q[1];
            double *fs = out.frame_stats + 4 * (size_t)f;
            fs[0] = m1 > 0 ? sqrt(s1 / (double)m1) : 0.0;
            fs[1] = m2 > 0 ? sqrt(s2 / (double)m2) : 0.0;
            fs[2] = m1 + m2 > 0 ? sqrt((s1 + s2) / (double)(m1 + m2)) : 0.0;
            fs[3] = rmax;
        }
    }
    __syncthreads();                                   // every wave has read the sums of the loop's last Jacobian pass
    if (lane == 0)
        for (int k = 0; k < MFPX_ST; k++) sSt3[wave * MFPX_ST + k] = gs[k];
    // one more Jacobian pass for N and frame_N (out.N and out.frame_N are the same for every wave); the barriers either way
    double U[21], gr[6], Rd[MFLM_SUMS];
    const bool want_N = out.N != nullptr || out.frame_N != nullptr;
    if (want_N) {
        prob.normal(x, U, gr);
        prob.template reduce<false>(0.0, Rd);
        if (out.frame_N)
            for (int kf = wave + WAVES * lane; kf < nk; kf += WAVES * 64) {
                double *fn = out.frame_N + MFJ_LOCAL * (size_t)sIdx[kf];
                for (int k = 0; k < MFJ_LOCAL; k++) fn[k] = prob.state(kf)[MFJ_V + k];
            }
    } else {
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double S1 = 0.0, S2 = 0.0, rmax = 0.0;
        for (int w = 0; w < WAVES; w++) {
            S1 = S1 + sSt3[w * MFPX_ST]; S2 = S2 + sSt3[w * MFPX_ST + 1]; rmax = fmax(rmax, sSt3[w * MFPX_ST + 2]);
        }
        for (int k = 0; k < 6; k++) out.x[6 * (size_t)g + k] = x[k];
        for (int k = 0; k < 16; k++) out.T[16 * (size_t)g + k] = Tf[k];
        out.fvals[2 * (size_t)g] = f0; out.fvals[2 * (size_t)g + 1] = fx;
        out.iters[2 * (size_t)g] = itercount; out.iters[2 * (size_t)g + 1] = func_evals;
        out.nused[g] = nk;
        for (int k = 0; k < 4; k++) out.counts[4 * (size_t)g + k] = cs[k];
        double *os = out.stats + 4 * (size_t)g;
        os[0] = cs[0] > 0 ? sqrt(S1 / (double)cs[0]) : 0.0;
        os[1] = cs[1] > 0 ? sqrt(S2 / (double)cs[1]) : 0.0;
        os[2] = sqrt((S1 + S2) / (double)nS);
        os[3] = rmax;
        if (out.N)
            for (int k = 0; k < 21; k++) out.N[21 * (size_t)g + k] = U[k] - Rd[k];
        out.status[g] = CPE_ST_OK;
    }
}
}  // namespace

extern "C" int32_t cpe_fit_cylinder_pixels_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                                 const int32_t *id2, const int32_t *cnt2, const double *cyl0, const uint8_t *use,
                                                 int32_t n, double radius, const double *K1, const double *K2, const double *T21,
                                                 const double *P, const int32_t *line_status, int32_t lo, int32_t hi,
                                                 const double *centre, int32_t swap, double min_cos, double gate_px, double tol_x,
                                                 double tol_f, int32_t max_iter, double *cyl, double *fvals, int32_t *iters,
                                                 int32_t *counts, double *stats, int32_t *status, double *res, int32_t *pt_state,
                                                 double *X, void *stream)
{
    CPE_CHECK_ARG(n >= 0, "cpe_fit_cylinder_pixels_batch: n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_fit_cylinder_pixels_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CPE_CHECK_ARG(radius > 0 && radius <= DBL_MAX, "cpe_fit_cylinder_pixels_batch: radius must be positive and finite");
    const struct { int swap; double min_cos, tol_x, tol_f; int max_iter; } p = {swap, min_cos, tol_x, tol_f, max_iter};
    CPE_CHECK_ARG(p.min_cos > 0 && p.min_cos < 1 && (p.swap == 0 || p.swap == 1) && p.tol_x > 0 && p.tol_f > 0 && p.max_iter >= 1,
                  "cpe_fit_cylinder_pixels_batch: bad parameters (0 < min_cos < 1, swap 0 or 1, tol_x > 0, tol_f > 0, max_iter >= 1)");
    const bool cam1 = xy1 && id1 && cnt1, cam2 = xy2 && id2 && cnt2;
    CPE_CHECK_ARG((cam1 || (!xy1 && !id1 && !cnt1)) && (cam2 || (!xy2 && !id2 && !cnt2)) && (cam1 || cam2),
                  "cpe_fit_cylinder_pixels_batch: a camera is given by all three of xy, id, cnt or by none, and one camera at least");
    if (n == 0) return CPE_OK;
    CPE_CHECK_ARG(cyl0 && K1 && K2 && T21 && P && line_status && centre && cyl && fvals && iters && counts && stats && status,
                  "cpe_fit_cylinder_pixels_batch: null pointer");
    const int L = hi - lo + 1;
    {
        const size_t N = (size_t)n, Pp = (size_t)CPE_MAXP;
        const struct { const void *p; size_t bytes; } buf[23] = {
            {xy1, cam1 ? N * Pp * 16 : 0}, {id1, cam1 ? N * Pp * 8 : 0}, {cnt1, cam1 ? N * 4 : 0}, {xy2, cam2 ? N * Pp * 16 : 0},
            {id2, cam2 ? N * Pp * 8 : 0}, {cnt2, cam2 ? N * 4 : 0}, {cyl0, N * 48}, {use, use ? N : 0}, {K1, 72}, {K2, 72}, {T21, 128},
            {P, (size_t)L * 64}, {line_status, (size_t)L * 8}, {centre, 24},
            {cyl, N * 48}, {fvals, N * 16}, {iters, N * 8}, {counts, N * 16}, {stats, N * 32}, {status, N * 4},
            {res, res ? N * Pp * 32 : 0}, {pt_state, pt_state ? N * Pp * 8 : 0}, {X, X ? N * Pp * 48 : 0}};
        for (int o = 14; o < 23; o++)
            for (int i = 0; i < o; i++)
                CPE_CHECK_ARG(!buf[o].bytes || !buf[i].bytes || !rl_overlap(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes),
                              "cpe_fit_cylinder_pixels_batch: an output overlaps an input or another output");
    }
    const PixOut out = {cyl, fvals, iters, counts, stats, status, res, pt_state, X};
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_fit_cylinder_pixels, dim3(n), dim3(64), 0, (hipStream_t)stream, xy1, id1, cnt1, xy2, id2, cnt2, cyl0, use, radius, K1, K2,
                T21, P, line_status, lo, L, centre, p.swap, p.min_cos, gate_px, p.tol_x, p.tol_f, p.max_iter, out);
    CPE_CHECK_LAUNCH("k_fit_cylinder_pixels");
    return CPE_OK;
}

extern "C" int32_t cpe_multi_frame_fit_pixels_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
                                                    const int32_t *id2, const int32_t *cnt2, const double *TAGVcyl,
                                                    const int32_t *frame_ok, const int32_t *group_start, int32_t G, int32_t n,
                                                    const double *x0_in, double radius, const double *K1, const double *K2,
                                                    const double *T21, const double *P, const int32_t *line_status, int32_t lo,
                                                    int32_t hi, const double *centre, int32_t swap, double min_cos, double sel_cos,
                                                    double gate_px, double tol_x, double tol_f, int32_t max_iter, double *x, double *T,
                                                    double *fvals, int32_t *iters, int32_t *n_used, int32_t *counts, double *stats,
                                                    int32_t *status, double *N, int32_t *pt_state, double *frame_cyl,
                                                    double *frame_stats, double *res, void *stream)
{
    CPE_CHECK_ARG(G >= 0 && n >= 0, "cpe_multi_frame_fit_pixels_batch: G < 0 or n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_multi_frame_fit_pixels_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CPE_CHECK_ARG(radius > 0 && radius <= DBL_MAX, "cpe_multi_frame_fit_pixels_batch: radius must be positive and finite");
    const struct { int swap; double min_cos, sel_cos, tol_x, tol_f; int max_iter; } p = {swap, min_cos, sel_cos, tol_x, tol_f, max_iter};
    CPE_CHECK_ARG(p.min_cos > 0 && p.min_cos < 1 && (p.swap == 0 || p.swap == 1) && p.tol_x > 0 && p.tol_f > 0 && p.max_iter >= 1,
                  "cpe_multi_frame_fit_pixels_batch: bad parameters (0 < min_cos < 1, swap 0 or 1, tol_x > 0, tol_f > 0, max_iter >= 1)");
    CPE_CHECK_ARG(p.sel_cos >= p.min_cos && p.sel_cos < 1, "cpe_multi_frame_fit_pixels_batch: sel_cos must lie in [min_cos, 1)");
    const bool cam1 = xy1 && id1 && cnt1, cam2 = xy2 && id2 && cnt2;
    CPE_CHECK_ARG((cam1 || (!xy1 && !id1 && !cnt1)) && (cam2 || (!xy2 && !id2 && !cnt2)) && (cam1 || cam2),
                  "cpe_multi_frame_fit_pixels_batch: a camera is given by all three of xy, id, cnt or by none, and one camera at least");
    if (G == 0) return CPE_OK;
    CPE_CHECK_ARG(TAGVcyl && group_start && x0_in && K1 && K2 && T21 && P && line_status && centre && x && T && fvals && iters && n_used &&
                      counts && stats && status && pt_state && frame_cyl && frame_stats,
                  "cpe_multi_frame_fit_pixels_batch: null pointer (x0_in is required: there is no closed-form start in pixel space)");
    const int L = hi - lo + 1;
    {
        const size_t Nn = (size_t)n, Gg = (size_t)G, Pp = (size_t)CPE_MAXP;
        const struct { const void *p; size_t bytes; } buf[29] = {
            {xy1, cam1 ? Nn * Pp * 16 : 0}, {id1, cam1 ? Nn * Pp * 8 : 0}, {cnt1, cam1 ? Nn * 4 : 0}, {xy2, cam2 ? Nn * Pp * 16 : 0},
            {id2, cam2 ? Nn * Pp * 8 : 0}, {cnt2, cam2 ? Nn * 4 : 0}, {TAGVcyl, Nn * 128}, {frame_ok, frame_ok ? Nn * 4 : 0},
            {group_start, (Gg + 1) * 4}, {x0_in, Gg * 48}, {K1, 72}, {K2, 72}, {T21, 128}, {P, (size_t)L * 64},
            {line_status, (size_t)L * 8}, {centre, 24},
            {x, Gg * 48}, {T, Gg * 128}, {fvals, Gg * 16}, {iters, Gg * 8}, {n_used, Gg * 4}, {counts, Gg * 16}, {stats, Gg * 32},
            {status, Gg * 4}, {N, N ? Gg * 168 : 0}, {pt_state, Nn * Pp * 8}, {frame_cyl, Nn * 48}, {frame_stats, Nn * 32},
            {res, res ? Nn * Pp * 32 : 0}};
        for (int o = 16; o < 29; o++)
            for (int i = 0; i < o; i++)
                CPE_CHECK_ARG(!buf[o].bytes || !buf[i].bytes || !rl_overlap(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes),
                              "cpe_multi_frame_fit_pixels_batch: an output overlaps an input or another output");
    }
    const MultiPixOut out = {x, T, fvals, iters, n_used, counts, stats, status, N, pt_state, frame_cyl, frame_stats, res};
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_multi_frame_pixels<MFPX_WAVES>, dim3(G), dim3(64 * MFPX_WAVES), 0, (hipStream_t)stream, xy1, id1, cnt1, xy2, id2, cnt2,
                TAGVcyl, frame_ok, group_start, n, x0_in, radius, K1, K2, T21, P, line_status, lo, L, centre, p.swap, p.min_cos, p.sel_cos,
                gate_px, p.tol_x, p.tol_f, p.max_iter, out);
    CPE_CHECK_LAUNCH("k_multi_frame_pixels");
    return CPE_OK;
}

extern "C" int32_t cpe_multi_frame_fit_pixels_angles_batch(const double *xy1, const int32_t *id1, const int32_t *cnt1, const double *xy2,
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
                                                           void *stream)
{
    CPE_CHECK_ARG(G >= 0 && n >= 0, "cpe_multi_frame_fit_pixels_angles_batch: G < 0 or n < 0");
    CPE_CHECK_ARG((long long)hi - (long long)lo + 1 >= 1 && (long long)hi - (long long)lo + 1 <= CPE_MAXL,
                  "cpe_multi_frame_fit_pixels_angles_batch: hi - lo + 1 must be 1..%d", CPE_MAXL);
    CPE_CHECK_ARG(radius > 0 && radius <= DBL_MAX, "cpe_multi_frame_fit_pixels_angles_batch: radius must be positive and finite");
    CPE_CHECK_ARG(w_pan > 0 && w_pan <= DBL_MAX && w_tilt > 0 && w_tilt <= DBL_MAX,
                  "cpe_multi_frame_fit_pixels_angles_batch: w_pan and w_tilt must be positive and finite");
    const struct { int swap; double min_cos, sel_cos, tol_x, tol_f; int max_iter; } p = {swap, min_cos, sel_cos, tol_x, tol_f, max_iter};
    CPE_CHECK_ARG(p.min_cos > 0 && p.min_cos < 1 && (p.swap == 0 || p.swap == 1) && p.tol_x > 0 && p.tol_f > 0 && p.max_iter >= 1,
                  "cpe_multi_frame_fit_pixels_angles_batch: bad parameters (0 < min_cos < 1, swap 0 or 1, tol_x > 0, tol_f > 0, max_iter >= 1)");
    CPE_CHECK_ARG(p.sel_cos >= p.min_cos && p.sel_cos < 1, "cpe_multi_frame_fit_pixels_angles_batch: sel_cos must lie in [min_cos, 1)");
    const bool cam1 = xy1 && id1 && cnt1, cam2 = xy2 && id2 && cnt2;
    CPE_CHECK_ARG((cam1 || (!xy1 && !id1 && !cnt1)) && (cam2 || (!xy2 && !id2 && !cnt2)) && (cam1 || cam2),
                  "cpe_multi_frame_fit_pixels_angles_batch: a camera is given by all three of xy, id, cnt or by none, and one camera at least");
    if (G == 0) return CPE_OK;
    CPE_CHECK_ARG(angles0 && group_start && x0_in && K1 && K2 && T21 && P && line_status && centre && x && T && fvals && iters && n_used &&
                      counts && stats && status && pt_state && frame_cyl && frame_stats && angles,
                  "cpe_multi_frame_fit_pixels_angles_batch: null pointer (x0_in is required: there is no closed-form start in pixel space)");
    const int L = hi - lo + 1;
    {
        const size_t Nn = (size_t)n, Gg = (size_t)G, Pp = (size_t)CPE_MAXP;
        const struct { const void *p; size_t bytes; } buf[31] = {
            {xy1, cam1 ? Nn * Pp * 16 : 0}, {id1, cam1 ? Nn * Pp * 8 : 0}, {cnt1, cam1 ? Nn * 4 : 0}, {xy2, cam2 ? Nn * Pp * 16 : 0},
            {id2, cam2 ? Nn * Pp * 8 : 0}, {cnt2, cam2 ? Nn * 4 : 0}, {angles0, Nn * 16}, {frame_ok, frame_ok ? Nn * 4 : 0},
            {group_start, (Gg + 1) * 4}, {x0_in, Gg * 48}, {K1, 72}, {K2, 72}, {T21, 128}, {P, (size_t)L * 64},
            {line_status, (size_t)L * 8}, {centre, 24},
            {x, Gg * 48}, {T, Gg * 128}, {fvals, Gg * 16}, {iters, Gg * 8}, {n_used, Gg * 4}, {counts, Gg * 16}, {stats, Gg * 32},
            {status, Gg * 4}, {N, N ? Gg * 168 : 0}, {pt_state, Nn * Pp * 8}, {frame_cyl, Nn * 48}, {frame_stats, Nn * 32},
            {res, res ? Nn * Pp * 32 : 0}, {angles, Nn * 16}, {frame_N, frame_N ? Nn * 136 : 0}};
        for (int o = 16; o < 31; o++)
            for (int i = 0; i < o; i++)
                CPE_CHECK_ARG(!buf[o].bytes || !buf[i].bytes || !rl_overlap(buf[o].p, buf[o].bytes, buf[i].p, buf[i].bytes),
                              "cpe_multi_frame_fit_pixels_angles_batch: an output overlaps an input or another output");
    }
    const MultiJointOut out = {{x, T, fvals, iters, n_used, counts, stats, status, N, pt_state, frame_cyl, frame_stats, res}, angles, frame_N};
    CPE_LAUNCH_BEGIN();
    CPE_KLAUNCH(k_multi_frame_pixels_angles<MFJ_WAVES>, dim3(G), dim3(64 * MFJ_WAVES), 0, (hipStream_t)stream, xy1, id1, cnt1, xy2, id2,
                cnt2, angles0, frame_ok, group_start, n, x0_in, w_pan, w_tilt, radius, K1, K2, T21, P, line_status, lo, L, centre, p.swap,
                p.min_cos, p.sel_cos, gate_px, p.tol_x, p.tol_f, p.max_iter, out);
    CPE_CHECK_LAUNCH("k_multi_frame_pixels_angles");
    return CPE_OK;
}
