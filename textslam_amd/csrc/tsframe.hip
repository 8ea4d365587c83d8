// libtsframe.so -- BA pyramid, gradient planes, per-level feature selection and INTERVAL8 reference intensities on gfx950
// (include/tsframe.h).  Integer image arithmetic is exact; the fp64 sampling is compiled without FMA
// contraction so that it rounds like the CPU restatement (oracle/tsframe_oracle.c).  Everything here is HBM-bound byte work:
// one thread per output pixel with coalesced rows, no LDS tiling needed at 640x480 (the 5x5 / 3x3 footprints live in L2).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/tsframe.h"
#include "tsraster.h"
#include "tsquadstat.h"
#include "tsstage.h"

struct FCtx {
    int device = 0; hipStream_t stream = nullptr; std::string err;
    int n_levels = 0, w[TSFRAME_MAX_LEVELS] = {0}, h[TSFRAME_MAX_LEVELS] = {0};
    uint8_t *plane[4][TSFRAME_MAX_LEVELS] = {{nullptr}};     // device planes: img, grad, gx, gy
    // blocks that only grow (tsstage.h):
    DeviceBlock plane_base;
    PinnedBlock h_stage;                // pinned staging (image in, results out)
    DeviceBlock d_work;                 // device block of the feature calls
    int cam_w = 0, cam_h = 0; int16_t *map_xy = nullptr; uint16_t *map_frac = nullptr;      // tsframe_set_camera: the fixed-point undistortion map (tsundist.h)
    DeviceBlock d_raw, d_col;               // tsframe_set_raw_image: the staged raw frame, the undistorted colour plane
};
#define CKF(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { c->err = std::string(#x) + ": " + hipGetErrorString(e_); return TSFRAME_ERR_DEVICE; } } while (0)

__device__ __forceinline__ int reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) { if (p < 0) p = -p; else p = 2*n - 2 - p; }
    return p;
}

// cv::pyrDown (8U): [1 4 6 4 1] x [1 4 6 4 1], BORDER_REFLECT_101, (sum + 128) >> 8
__global__ __launch_bounds__(256) void k_pyrdown(const uint8_t *__restrict__ src, int w, int h, uint8_t *__restrict__ dst, int dw, int dh) {
    const int x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    int xs[5];
#pragma unroll
    for (int k = 0; k < 5; k++) xs[k] = reflect101(2*x - 2 + k, w);
    const int wk[5] = { 1, 4, 6, 4, 1 };
    int sum = 0;
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const uint8_t *s = src + (size_t)reflect101(2*y - 2 + r, h)*w;
        sum += wk[r]*(s[xs[0]] + 4*s[xs[1]] + 6*s[xs[2]] + 4*s[xs[3]] + s[xs[4]]);
    }
    dst[(size_t)y*dw + x] = (uint8_t)((sum + 128) >> 8);
}

// cv::Sobel x / y (CV_8U: saturating) and addWeighted(.5, .5) (float, round half to even)
__global__ __launch_bounds__(256) void k_gradients(const uint8_t *__restrict__ src, int w, int h, uint8_t *__restrict__ gx, uint8_t *__restrict__ gy, uint8_t *__restrict__ grad) {
    const int x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t *r0 = src + (size_t)reflect101(y - 1, h)*w, *r1 = src + (size_t)y*w, *r2 = src + (size_t)reflect101(y + 1, h)*w;
    const int xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
    const int sx = (r0[xp] - r0[xm]) + 2*(r1[xp] - r1[xm]) + (r2[xp] - r2[xm]);
    const int sy = (r2[xm] - r0[xm]) + 2*(r2[x] - r0[x]) + (r2[xp] - r0[xp]);
    const int a = min(max(sx, 0), 255), b = min(max(sy, 0), 255), s = a + b;
    gx[(size_t)y*w + x] = (uint8_t)a; gy[(size_t)y*w + x] = (uint8_t)b;
    grad[(size_t)y*w + x] = (uint8_t)((s & 1) ? ((s >> 1) + ((s >> 1) & 1)) : (s >> 1));
}

// tool::GetIntenBilinterPtr (reads of zero-weight neighbours past the image are clamped: they do not change the value)
__device__ __forceinline__ bool bilinear(const uint8_t *__restrict__ img, int w, int h, double u, double v, double &out) {
    const int x0 = (int)floor(u), y0 = (int)floor(v), x1 = (int)ceil(u), y1 = (int)ceil(v);
    if (x0 < 0 || y0 < 0 || x1 >= w || y1 >= h) { out = 0.0; return false; }
    const double a = u - x0, b = v - y0;
    const double wtl = (1.0 - a)*(1.0 - b), wtr = a*(1.0 - b), wbl = (1.0 - a)*b, wbr = a*b;
    const int xr = min(x0 + 1, w - 1), yb = min(y0 + 1, h - 1);
    const double p00 = img[(size_t)y0*w + x0], p01 = img[(size_t)y0*w + xr], p10 = img[(size_t)yb*w + x0], p11 = img[(size_t)yb*w + xr];
    out = wtl*p00 + wtr*p01 + wbl*p10 + wbr*p11;
    return true;
}

struct GridDev { int mode, cw, ch; double s, x0, y0, fx, fy; };

__device__ __constant__ double NB_DX[8] = { 0, 2, 1, 0, -1, -2, -1, 0 };
__device__ __constant__ double NB_DY[8] = { 0, 0, -1, -2, -1, 0, 1, 2 };
// tool::GetNeighbour(INTERVAL8): thread = (feature, tap)
__global__ __launch_bounds__(256) void k_neighbours(const uint8_t *__restrict__ img, int w, int h, const double *__restrict__ uv, int n, double mu, double sigma,
                                                    double *inten8, double *ninten8, uint8_t *in) {
    const int e = blockIdx.x*256 + threadIdx.x, j = e >> 3, k = e & 7;
    if (j >= n) return;
    double I; const bool ok = bilinear(img, w, h, uv[2*j] + NB_DX[k], uv[2*j + 1] + NB_DY[k], I);
    inten8[e] = I; ninten8[e] = (I - mu)/sigma;
    if (k == 7) in[j] = ok ? 1 : 0;                            // feat->IN keeps the flag of the last tap
}

// ------------------------------------------------------------------------------------------------ host side
// Ordered compaction of one tile by a workgroup of NWAVES waves (k_box_pixels, k_pts_batch, k_object_info): the slot of a hit = base + the hits of the lower
// waves (s_w [NWAVES]) + the hits of the lower lanes (ballot); base advances by the tile's total.  Every thread of the workgroup calls it: the two
// barriers are those around s_w.  The slot of a miss means nothing.
template <int NWAVES>
__device__ __forceinline__ int wg_ordered_slot(bool hit, int *s_w, int &base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int q = 0; q < NWAVES; q++) { const int c = s_w[q]; if (q < wave) off += c; tot += c; }
    base += tot;
    __syncthreads();
    return off + __popcll(bal & ((1ull << lane) - 1ull));
}
// ---- tool::GetBoxAllPixs (tool.cc:1264-1337): every pixel of the level image inside the filled detection quad, in row-major order
// of the clamped bounding box.  One workgroup: scan conversion of the quad into a bit mask (cv::fillPoly semantics, tsraster.h), then an
// ordered compaction of the box in tiles of 1024 pixels (wg_ordered_slot).
struct BoxDev { int xy[8]; int x0, x1, y0, y1; };
__global__ __launch_bounds__(1024) void k_box_pixels(const uint8_t *__restrict__ img, int w, int h, BoxDev B, double mu, double sigma, unsigned *mask,
                                                     int *cnt, int *__restrict__ u, int *__restrict__ v, double *__restrict__ inten, double *__restrict__ ninten) {
    __shared__ int s_xy[8], s_w[16];
    const int tid = threadIdx.x;
    if (tid < 8) s_xy[tid] = B.xy[tid];
    for (int k = tid; k < (w*h + 31) >> 5; k += 1024) mask[k] = 0;
    __syncthreads();
    raster_quad(mask, s_xy, w, h, tid, 1024);
    __syncthreads();
    const int bw = B.x1 - B.x0 + 1, bh = B.y1 - B.y0 + 1, npx = bw*bh;
    int base = 0;
    for (int k0 = 0; k0 < npx; k0 += 1024) {
        const int k = k0 + tid;
        int x = 0, y = 0; bool in = false;
        if (k < npx) { x = B.x0 + k % bw; y = B.y0 + k / bw; const int bit = y*w + x; in = (mask[bit >> 5] >> (bit & 31)) & 1u; }
        const int at = wg_ordered_slot<16>(in, s_w, base);
        if (in) {
            const double I = (double)img[y*w + x];
            u[at] = x; v[at] = y; inten[at] = I; ninten[at] = (I - mu)/sigma;
        }
    }
    if (tid == 0) *cnt = base;
}

// ---- tracking::TextJudgeSingle (tracking.cc:1991-2131) for a batch of planes: one workgroup per plane, no waits between workgroups, so a
// plane's outputs do not depend on its neighbours or its position in the batch.  Thread 0 takes the orientation and the four corners
// (tool::CheckOrientation, GetProjText of vTextDeteRay); then three strided sweeps over the plane's reference pixels with fixed-order block
// sums (means, centred variances, products of the normalised samples: tool::CheckZNCC -> VectorNorm -> CalZNCC without its unused top
// fractions); then, for a plane that passed, cv::fillPoly of the projected quad into an LDS bit mask (raster_quad) tested at the rounded
// detection centres.  The current-image samples of the first JUDGE_CACHE pixels stay in LDS between the sweeps, the rest are recomputed
// (same code, same bits); the cache and the mask share the same LDS.
#define JUDGE_NT 256
#ifndef JUDGE_CACHE
#define JUDGE_CACHE (MS_MASK_WORDS/2)                           /* doubles: the union with the label mask, 38.4 KB (-DJUDGE_CACHE=0: recompute every sweep) */
#endif
struct JudgePlane { double theta[3], T[12], ray[8]; };          // in: one plane (184 B)
struct JudgeOut { double cos, zncc, box[8]; int32_t reason, pad; };   // out: one plane (88 B)
struct JudgeArgs {
    int w, h, w0, h0, margin, n_dete, dete_words; double Kr[4], K[4], cos_min, zncc_min;
};

// tool::GetProjText (Mat31 overload, tool.cc:1593) of the reference pixel (u, v) and tool::GetIntenBilinterPtr on the current level image: the
// depth's sign is ignored, a sample outside the image (or at a NaN position, which the reference's int conversion sends below 0) gives 0.
__device__ __forceinline__ double judge_sample(const uint8_t *__restrict__ img, const JudgeArgs &A, const double *th, const double *T, int u, int v) {
    const double r0 = ((double)u - A.Kr[2])/A.Kr[0], r1 = ((double)v - A.Kr[3])/A.Kr[1], r2 = 1.0;
    const double invz = -(r0*th[0] + r1*th[1] + r2*th[2]);
    const double X = (T[0]*r0 + T[1]*r1 + T[2]*r2)/invz + T[3];
    const double Y = (T[4]*r0 + T[5]*r1 + T[6]*r2)/invz + T[7];
    const double Z = (T[8]*r0 + T[9]*r1 + T[10]*r2)/invz + T[11];
    const double pu = A.K[0]*X/Z + A.K[2], pv = A.K[1]*Y/Z + A.K[3];
    double I = 0.0;
    if (pu == pu && pv == pv) bilinear(img, A.w, A.h, pu, pv, I);
    return I;
}

// BIG (a level-0 image above MS_MASK_WORDS*32 pixels): no mask -- every rounded centre is tested with quad_covers, the same fill's point membership.
template <bool BIG>
__global__ __launch_bounds__(JUDGE_NT) void k_text_judge(const uint8_t *__restrict__ img, JudgeArgs A, const JudgePlane *__restrict__ planes,
                                                         const int *__restrict__ pix_off, const short *__restrict__ pix_uv,
                                                         const uint8_t *__restrict__ pix_inten, const double *__restrict__ dete_xy,
                                                         JudgeOut *__restrict__ out, unsigned *__restrict__ dete_bits) {
    __shared__ union { double cache[JUDGE_CACHE > 0 ? JUDGE_CACHE : 1]; unsigned mask[MS_MASK_WORDS]; } s_u;
    __shared__ double s_red[JUDGE_NT], s_th[3], s_T[12];
    __shared__ int s_reason, s_xy[8];
    const int tid = threadIdx.x, p = blockIdx.x;
    const JudgePlane &P = planes[p];
    if (tid < 3) s_th[tid] = P.theta[tid];
    if (tid < 12) s_T[tid] = P.T[tid];
    if (tid == 0) {
        const double *th = P.theta, *T = P.T;
        // 1. tool::CheckOrientation (tool.cc:1393-1407): c = third column of R_cr^T, norms as sqrt of the squared norms
        const double c0 = T[8], c1 = T[9], c2 = T[10];
        const double nv = sqrt(th[0]*th[0] + th[1]*th[1] + th[2]*th[2])*sqrt(c0*c0 + c1*c1 + c2*c2);
        const double cs = (th[0]*c0 + th[1]*c1 + th[2]*c2)/nv;
        int reason = fabs(cs) < A.cos_min ? TSFRAME_JUDGE_ORIENT : TSFRAME_JUDGE_PASS;
        // 2. the four corners (GetProjText, Vec2 overload, tool.cc:1608-1623): the first corner behind the camera or at the border decides
        for (int b = 0; b < 4; b++) {
            const double r0 = P.ray[2*b], r1 = P.ray[2*b + 1], r2 = 1.0;
            const double invz = -(r0*th[0] + r1*th[1] + r2*th[2]);
            const double X = (T[0]*r0 + T[1]*r1 + T[2]*r2)/invz + T[3];
            const double Y = (T[4]*r0 + T[5]*r1 + T[6]*r2)/invz + T[7];
            const double Z = (T[8]*r0 + T[9]*r1 + T[10]*r2)/invz + T[11];
            const double u = A.K[0]*X/Z + A.K[2], v = A.K[1]*Y/Z + A.K[3];
            out[p].box[2*b] = u; out[p].box[2*b + 1] = v;
            s_xy[2*b] = (u > -1e9 && u < 1e9) ? (int)u : 0; s_xy[2*b + 1] = (v > -1e9 && v < 1e9) ? (int)v : 0;   // cv::Point truncation (used only if passed)
            if (reason == TSFRAME_JUDGE_PASS) {
                if (Z < 0) reason = TSFRAME_JUDGE_DEPTH;
                else if (u <= (double)A.margin || u >= (double)(A.w - A.margin) || v <= (double)A.margin || v >= (double)(A.h - A.margin)) reason = TSFRAME_JUDGE_BOX;
            }
        }
        out[p].cos = cs;
        s_reason = reason;
    }
    __syncthreads();
    int reason = s_reason;                                      // (every thread: the branches below are uniform in the workgroup)
    double zncc = __builtin_nan("");
    // 3. tool::CheckZNCC: ref = featureInten, cur = the bilinear samples; mean, sample std (n - 1), mean of the normalised products
    if (reason == TSFRAME_JUDGE_PASS && A.zncc_min > -2.0) {
        const int i0 = pix_off[p], n = pix_off[p + 1] - i0;
        if (n >= 2) {
            double sr = 0.0, sc = 0.0;
            for (int i = tid; i < n; i += JUDGE_NT) {
                const double c = judge_sample(img, A, s_th, s_T, pix_uv[2*(i0 + i)], pix_uv[2*(i0 + i) + 1]);
                if (i < JUDGE_CACHE) s_u.cache[i] = c;
                sr += (double)pix_inten[i0 + i]; sc += c;
            }
            const double mr = block_sum<JUDGE_NT>(sr, s_red)/(double)n, mc = block_sum<JUDGE_NT>(sc, s_red)/(double)n;
            double vr = 0.0, vc = 0.0;
            for (int i = tid; i < n; i += JUDGE_NT) {
                const double c = i < JUDGE_CACHE ? s_u.cache[i] : judge_sample(img, A, s_th, s_T, pix_uv[2*(i0 + i)], pix_uv[2*(i0 + i) + 1]);
                const double r = (double)pix_inten[i0 + i];
                vr += (r - mr)*(r - mr); vc += (c - mc)*(c - mc);
            }
            const double sdr = sqrt(block_sum<JUDGE_NT>(vr, s_red)/(double)(n - 1)), sdc = sqrt(block_sum<JUDGE_NT>(vc, s_red)/(double)(n - 1));
            if (sdr != 0.0 && sdc != 0.0) {
                double sp = 0.0;
                for (int i = tid; i < n; i += JUDGE_NT) {
                    const double c = i < JUDGE_CACHE ? s_u.cache[i] : judge_sample(img, A, s_th, s_T, pix_uv[2*(i0 + i)], pix_uv[2*(i0 + i) + 1]);
                    const double r = (double)pix_inten[i0 + i];
                    sp += ((r - mr)/sdr)*((c - mc)/sdc);
                }
                zncc = block_sum<JUDGE_NT>(sp, s_red)/(double)n;
            } else {
                zncc = -100.0;
            }
        }
        if (!(zncc >= A.zncc_min)) reason = TSFRAME_JUDGE_ZNCC;   // (n < 2: NaN)
        __syncthreads();                                        // (the cache is done before the mask reuses it)
    }
    if (tid == 0) { out[p].zncc = zncc; out[p].reason = reason; out[p].pad = 0; }
    // 4. detection association (tracking.cc:2116-2128): label image = the quad filled by cv::fillPoly; centre (round(u), round(v)), half away from zero
    if (dete_bits && A.dete_words > 0) {
        unsigned *bits = dete_bits + (size_t)p*A.dete_words;
        if constexpr (!BIG)
            if (reason == TSFRAME_JUDGE_PASS) {
                for (int k = tid; k < (A.w0*A.h0 + 31) >> 5; k += JUDGE_NT) s_u.mask[k] = 0;
                __syncthreads();
                raster_quad(s_u.mask, s_xy, A.w0, A.h0, tid, JUDGE_NT);
                __syncthreads();
            }
        for (int k = tid; k < A.dete_words; k += JUDGE_NT) {
            unsigned word = 0;
            if (reason == TSFRAME_JUDGE_PASS)
                for (int j = 32*k; j < min(32*k + 32, A.n_dete); j++) {
                    const double ru = round(dete_xy[2*j]), rv = round(dete_xy[2*j + 1]);
                    if (!(ru >= 0.0 && ru <= (double)(A.w0 - 1) && rv >= 0.0 && rv <= (double)(A.h0 - 1))) continue;
                    bool in;
                    if constexpr (BIG) in = quad_covers(s_xy, A.w0, A.h0, (int)ru, (int)rv);
                    else { const int bit = (int)rv*A.w0 + (int)ru; in = (s_u.mask[bit >> 5] >> (bit & 31)) & 1u; }
                    if (in) word |= 1u << (j & 31);
                }
            bits[k] = word;
        }
    }
}

#include "tsklt.h"
#include "tspts.h"
#include "tsobj.h"
#include "tsundist.h"

// The feature calls below stage through tsstage.h: one Layout over [in || out] serves the pinned block (c->h_stage) and the device block (c->d_work), a take per
// sub-array of the call's layout comment.  Both blocks are grown to the layout's end; the copy up is the inputs, the copy down starts at the first output.

// The corners of quad * scale as cv::Point(double, double) (truncation) and their clamped bounding box, statement by statement as tool.cc:1269-1298: min / max
// on strict improvement from w + 1 / -1, then the eight clamps in the reference's order.  An empty box has x1 < x0 or y1 < y0.
static void quad_box(const double *quad, double scale, int w, int h, int xy[8], int &x0, int &x1, int &y0, int &y1) {
    int xMin = w + 1, xMax = -1, yMin = h + 1, yMax = -1;
    for (int i = 0; i < 4; i++) {
        const double x = quad[2*i]*scale, y = quad[2*i + 1]*scale;
        xy[2*i] = (int)x; xy[2*i + 1] = (int)y;
        if (x > xMax) xMax = (int)ceil(x);
        if (x < xMin) xMin = (int)floor(x);
        if (y > yMax) yMax = (int)ceil(y);
        if (y < yMin) yMin = (int)floor(y);
    }
    if (xMin < 0) xMin = 0;
    if (xMin >= w) xMin = w - 1;
    if (yMin < 0) yMin = 0;
    if (yMin >= h) yMin = h - 1;
    if (xMax >= w) xMax = w - 1;
    if (xMax < 0) xMax = 0;
    if (yMax >= h) yMax = h - 1;
    if (yMax < 0) yMax = 0;
    x0 = xMin; x1 = xMax; y0 = yMin; y1 = yMax;
}

// the cell grid of level l >= 1 for a set of n raw features (host doubles, the reference's expressions: tool.cc:599-616 / :898-907);
// false: degenerate (cw < 1 or ch < 1)
static bool pts_grid(const FCtx *c, int mode, int n, const double *box, int l, double s, GridDev &g) {
    const size_t ncell = (size_t)((double)n*s*s + (mode == 0 ? 100 : 500));
    g.mode = mode; g.s = s; g.x0 = 0.0; g.y0 = 0.0;
    if (mode == 0) {
        const double pminx = box[0]*s, pminy = box[1]*s, pmaxx = box[2]*s, pmaxy = box[3]*s;
        const double WH = (pmaxx - pminx)/(pmaxy - pminy);
        g.ch = (int)sqrt((double)ncell/WH); g.cw = (int)sqrt((double)ncell*WH);
        g.fx = (pmaxx - pminx)/(double)g.cw; g.fy = (pmaxy - pminy)/(double)g.ch;
        g.x0 = pminx; g.y0 = pminy;
    } else {
        const double WH = (double)c->w[l]/(double)c->h[l];
        g.ch = (int)sqrt((double)ncell/WH); g.cw = (int)sqrt((double)ncell*WH);
        g.fx = (double)c->w[l]/(double)g.cw; g.fy = (double)c->h[l]/(double)g.ch;
    }
    return g.cw >= 1 && g.ch >= 1;
}

// GetPyramidPts on the device, for tsframe_pyramid_pts (one set) and tsframe_pyramid_pts_batch.  pts_set_jobs: the L jobs of one set of n features that
// starts at feature xy0, level-major, with the LDS / scratch choice per level (sel_ints: the scratch handed out so far); returns the reason of a refusal,
// which the caller words for its entry point, or NULL.  Both refusals protect memory: the kernel's int indices rest on them, and on the caller's bound
// of INT32_MAX / L features in all, which out0 needs.
static const char *pts_set_jobs(const FCtx *c, int mode, int xy0, int n, const double *box, const double *inv_scale, PtsJob *jobs, size_t &sel_ints) {
    const int L = c->n_levels;
    for (int l = 0; l < L; l++) {
        PtsJob &J = jobs[l];
        J.G = GridDev{mode, 1, 1, 1.0, 0, 0, 1, 1};
        if (l > 0 && !pts_grid(c, mode, n, box, l, inv_scale[l], J.G)) return "degenerate feature grid (empty box?)";
        const size_t ncell = (size_t)J.G.cw*(size_t)J.G.ch;
        if (ncell > (size_t)INT32_MAX) return "feature grid above 2^31 cells";
        J.img = c->plane[TSFRAME_IMG][l]; J.grad = c->plane[TSFRAME_GRAD][l]; J.w = c->w[l]; J.h = c->h[l];
        J.level = l; J.xy0 = xy0; J.n = n; J.out0 = xy0*L + l*n;
        J.sel_off = -1;
        if (l > 0 && n > 0 && ncell > PTS_LDS_CELLS) { J.sel_off = (long long)sel_ints; sel_ints += ncell; }
    }
    return nullptr;
}
// pts_run: the jobs of n_set sets (pts_set_jobs) as one block up, one launch of k_pts_batch, one copy back, and the packing copy-out
static int pts_run(FCtx *c, int n_set, const int32_t *xy_off, const float *xy, const std::vector<PtsJob> &jobs, size_t sel_ints,
                   int32_t *level_off, double *u, double *v, int32_t *idx, double *inten, uint8_t *in) {
    const int L = c->n_levels;
    const size_t total = (size_t)xy_off[n_set];
    if (total == 0) { memset(level_off, 0, sizeof(int32_t)*(size_t)n_set*(L + 1)); return TSFRAME_OK; }
    hipSetDevice(c->device);
    // one block, inputs then outputs: jobs | xy || cnt | u | v | inten | idx | in; then the large grids' scratch (device only)
    const size_t cap = total*L;
    Layout S(256);
    const auto a_job = S.take<PtsJob>(jobs.size()); const auto a_xy = S.take<float>(2*total);
    const size_t in_end = S.mark();
    const auto a_cnt = S.take<int32_t>(jobs.size()); const auto a_u = S.take<double>(cap), a_v = S.take<double>(cap), a_I = S.take<double>(cap);
    const auto a_idx = S.take<int32_t>(cap); const auto a_in = S.take<uint8_t>(cap);
    const size_t tot = S.mark();
    const auto a_sel = S.take<int32_t>(sel_ints);
    CKF(c->d_work.grow(S.mark())); CKF(c->h_stage.grow(tot));
    void *h = c->h_stage.as(), *d = c->d_work.as();
    a_job.put(h, jobs.data()); a_xy.put(h, xy);
    CKF(hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pts_batch, dim3((unsigned)a_job.n), dim3(PTS_NT), 0, c->stream, a_job.at(d), a_xy.at(d), a_sel.at(d), a_cnt.at(d),
                       a_u.at(d), a_v.at(d), a_idx.at(d), a_I.at(d), a_in.at(d));
    CKF(hipGetLastError());
    CKF(hipMemcpyAsync(a_cnt.at(h), a_cnt.at(d), tot - in_end, hipMemcpyDeviceToHost, c->stream));
    CKF(hipStreamSynchronize(c->stream));
    // copy-out: level l of set i lies at out0 = xy_off[i]*L + l*n_i with cnt entries; packed behind the set's base
    const int32_t *cnt = a_cnt.at(h);
    for (int i = 0; i < n_set; i++) {
        int32_t *lo = level_off + (size_t)i*(L + 1);
        const size_t base = (size_t)xy_off[i]*L;
        lo[0] = 0;
        for (int l = 0; l < L; l++) {
            const size_t src = (size_t)jobs[(size_t)i*L + l].out0, dst = base + (size_t)lo[l], m = std::min((size_t)cnt[(size_t)i*L + l], (size_t)(xy_off[i + 1] - xy_off[i]));
            std::copy_n(a_u.at(h) + src, m, u + dst); std::copy_n(a_v.at(h) + src, m, v + dst); std::copy_n(a_I.at(h) + src, m, inten + dst);
            std::copy_n(a_idx.at(h) + src, m, idx + dst); std::copy_n(a_in.at(h) + src, m, in + dst);
            lo[l + 1] = lo[l] + (int32_t)m;
        }
    }
    return TSFRAME_OK;
}

// The four planes of every level in one allocation (frame::GetPyrMat's sizes: level l = ceil(level l-1 / 2)), kept while it is large enough.
static int planes_layout(FCtx *c, int w, int h, int n_levels) {
    size_t tot = 0; int lw = w, lh = h;
    for (int l = 0; l < n_levels; l++) { c->w[l] = lw; c->h[l] = lh; tot += ((size_t)lw*lh + 255) & ~(size_t)255; lw = (lw + 1)/2; lh = (lh + 1)/2; }
    CKF(c->plane_base.grow(4*tot));
    uint8_t *p = c->plane_base.as<uint8_t>();
    for (int k = 0; k < 4; k++) for (int l = 0; l < n_levels; l++) { c->plane[k][l] = p; p += ((size_t)c->w[l]*c->h[l] + 255) & ~(size_t)255; }
    c->n_levels = n_levels;
    return 0;
}
// frame::GetPyrMat from the level-0 image that the stream has been given: pyrDown per level, the gradient planes of every level; waits for all of it.
static int pyramid_from_level0(FCtx *c) {
    for (int l = 0; l < c->n_levels; l++) {
        if (l > 0) hipLaunchKernelGGL(k_pyrdown, dim3((c->w[l] + 63)/64, (c->h[l] + 3)/4), dim3(256), 0, c->stream,
                                      (const uint8_t *)c->plane[TSFRAME_IMG][l - 1], c->w[l - 1], c->h[l - 1], c->plane[TSFRAME_IMG][l], c->w[l], c->h[l]);
        hipLaunchKernelGGL(k_gradients, dim3((c->w[l] + 63)/64, (c->h[l] + 3)/4), dim3(256), 0, c->stream,
                           (const uint8_t *)c->plane[TSFRAME_IMG][l], c->w[l], c->h[l], c->plane[TSFRAME_GRADX][l], c->plane[TSFRAME_GRADY][l], c->plane[TSFRAME_GRAD][l]);
    }
    CKF(hipStreamSynchronize(c->stream)); CKF(hipGetLastError());
    return TSFRAME_OK;
}

extern "C" {

int tsframe_create(int device, void **ctx) {
    if (!ctx) return TSFRAME_ERR_ARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return TSFRAME_ERR_DEVICE;      // no GPU: fail loudly, no CPU path
    FCtx *c = new FCtx(); c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) { delete c; return TSFRAME_ERR_DEVICE; }
    *ctx = c; return TSFRAME_OK;
}
void tsframe_destroy(void *ctx) {
    FCtx *c = (FCtx *)ctx; if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    if (c->map_xy) hipFree(c->map_xy);
    if (c->map_frac) hipFree(c->map_frac);
    delete c;                               // the blocks go with the context
}
const char *tsframe_last_error(void *ctx) { FCtx *c = (FCtx *)ctx; return c ? c->err.c_str() : "null context"; }

int tsframe_set_image(void *ctx, const uint8_t *img, int w, int h, int n_levels) {
    FCtx *c = (FCtx *)ctx; if (!c || !img || w < 2 || h < 2 || n_levels < 1 || n_levels > TSFRAME_MAX_LEVELS) return TSFRAME_ERR_ARG;
    hipSetDevice(c->device);
    int rc = planes_layout(c, w, h, n_levels); if (rc) return rc;
    CKF(c->h_stage.grow((size_t)w*h));
    memcpy(c->h_stage.as(), img, (size_t)w*h);
    CKF(hipMemcpyAsync(c->plane[TSFRAME_IMG][0], c->h_stage.as(), (size_t)w*h, hipMemcpyHostToDevice, c->stream));
    return pyramid_from_level0(c);
}

/* cv::undistort's map for one camera (docs/undistort_recalled.md U1 - U5), kept on the device until the next call.  The new map is built beside the old
 * one and takes its place only when the kernel has finished. */
int tsframe_set_camera(void *ctx, int w, int h, const double K[4], const double dist[5], const double K_new[4]) {
    FCtx *c = (FCtx *)ctx; if (!c) return TSFRAME_ERR_ARG;
    auto bad = [&](const char *m) { c->err = std::string("tsframe_set_camera: ") + m; return TSFRAME_ERR_ARG; };
    if (!K || !dist) return bad("K or dist is NULL");
    if (w < 2 || h < 2 || w > 8192 || h > 8192) return bad("w or h outside [2, 8192]");
    const double *Kn = K_new ? K_new : K;
    for (int i = 0; i < 4; i++) if (!std::isfinite(K[i]) || !std::isfinite(Kn[i])) return bad("K or K_new is not finite");
    for (int i = 0; i < 5; i++) if (!std::isfinite(dist[i])) return bad("dist is not finite");
    if (K[0] == 0.0 || K[1] == 0.0 || Kn[0] == 0.0 || Kn[1] == 0.0) return bad("fx or fy is 0 (K or K_new)");
    hipSetDevice(c->device);
    UndistCam C; memcpy(C.K, K, sizeof(C.K)); memcpy(C.dist, dist, sizeof(C.dist)); memcpy(C.Kn, Kn, sizeof(C.Kn));
    C.w = w; C.h = h; C.s0 = std::min(std::max(1, 4096/std::max(w, 1)), h);
    const size_t n4 = ((size_t)w*h + 3) & ~(size_t)3;            // (k_undist_grey loads four entries at a time)
    int16_t *xy = nullptr; uint16_t *fr = nullptr;
    CKF(hipMalloc((void **)&xy, n4*2*sizeof(int16_t)));
    if (hipMalloc((void **)&fr, n4*sizeof(uint16_t)) != hipSuccess) { hipFree(xy); c->err = "tsframe_set_camera: hipMalloc failed"; return TSFRAME_ERR_DEVICE; }
    hipError_t e = hipMemsetAsync(xy, 0, n4*2*sizeof(int16_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(fr, 0, n4*sizeof(uint16_t), c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(k_undist_map, dim3((h + 63)/64), dim3(64), 0, c->stream, C, xy, fr); e = hipStreamSynchronize(c->stream); }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { hipFree(xy); hipFree(fr); c->err = std::string("tsframe_set_camera: ") + hipGetErrorString(e); return TSFRAME_ERR_DEVICE; }
    if (c->map_xy) hipFree(c->map_xy);
    if (c->map_frac) hipFree(c->map_frac);
    c->map_xy = xy; c->map_frac = fr; c->cam_w = w; c->cam_h = h;
    return TSFRAME_OK;
}

int tsframe_get_undist_map(void *ctx, int16_t *xy, uint16_t *frac) {
    FCtx *c = (FCtx *)ctx; if (!c) return TSFRAME_ERR_ARG;
    if (!xy || !frac) { c->err = "tsframe_get_undist_map: xy or frac is NULL"; return TSFRAME_ERR_ARG; }
    if (!c->map_xy) { c->err = "tsframe_get_undist_map: no camera set (tsframe_set_camera first)"; return TSFRAME_ERR_STATE; }
    hipSetDevice(c->device);
    const size_t n = (size_t)c->cam_w*c->cam_h;
    CKF(hipMemcpy(xy, c->map_xy, n*2*sizeof(int16_t), hipMemcpyDeviceToHost));
    CKF(hipMemcpy(frac, c->map_frac, n*sizeof(uint16_t), hipMemcpyDeviceToHost));
    return TSFRAME_OK;
}

/* cv::undistort + cvtColor + frame::GetPyrMat of one raw camera frame: one copy up, k_undist_grey writes level 0 (and the colour plane when asked),
 * then tsframe_set_image's own chain. */
int tsframe_set_raw_image(void *ctx, const uint8_t *raw, int stride, int format, int n_levels, uint8_t *undist_out) {
    FCtx *c = (FCtx *)ctx; if (!c) return TSFRAME_ERR_ARG;
    auto bad = [&](const char *m) { c->err = std::string("tsframe_set_raw_image: ") + m; return TSFRAME_ERR_ARG; };
    if (!raw) return bad("raw is NULL");
    if (format != TSFRAME_RAW_BGR && format != TSFRAME_RAW_RGB && format != TSFRAME_RAW_GREY) return bad("format is none of TSFRAME_RAW_BGR / RGB / GREY");
    if (n_levels < 1 || n_levels > TSFRAME_MAX_LEVELS) return bad("n_levels outside [1, 8]");
    if (!c->map_xy) { c->err = "tsframe_set_raw_image: no camera set (tsframe_set_camera first)"; return TSFRAME_ERR_STATE; }
    const int w = c->cam_w, h = c->cam_h, ch = format == TSFRAME_RAW_GREY ? 1 : 3;
    if (stride < w*ch) return bad("stride < w * channels");
    hipSetDevice(c->device);
    const size_t raw_bytes = (size_t)(h - 1)*stride + (size_t)w*ch, col_bytes = (size_t)w*h*ch;      // (the last row ends with its pixels)
    CKF(c->d_raw.grow(raw_bytes));
    if (undist_out) CKF(c->d_col.grow((col_bytes + 255) & ~(size_t)255));        // (whole dwords at the end of the plane)
    int rc = planes_layout(c, w, h, n_levels); if (rc) return rc;
    CKF(c->h_stage.grow(std::max(raw_bytes, col_bytes)));                          // the raw frame in, then the colour plane out
    memcpy(c->h_stage.as(), raw, raw_bytes);
    CKF(hipMemcpyAsync(c->d_raw.as(), c->h_stage.as(), raw_bytes, hipMemcpyHostToDevice, c->stream));
    const int npix = w*h; const dim3 grid((npix + 1023)/1024), block(256);
    const int r_first = format == TSFRAME_RAW_RGB;
    uint8_t *g0 = c->plane[TSFRAME_IMG][0];
    if (ch == 3) {
        if (undist_out) hipLaunchKernelGGL((k_undist_grey<3, true>), grid, block, 0, c->stream, c->d_raw.as<const uint8_t>(), w, h, stride, r_first, (const int16_t *)c->map_xy, (const uint16_t *)c->map_frac, npix, g0, c->d_col.as<uint8_t>());
        else hipLaunchKernelGGL((k_undist_grey<3, false>), grid, block, 0, c->stream, c->d_raw.as<const uint8_t>(), w, h, stride, r_first, (const int16_t *)c->map_xy, (const uint16_t *)c->map_frac, npix, g0, (uint8_t *)nullptr);
    } else {
        if (undist_out) hipLaunchKernelGGL((k_undist_grey<1, true>), grid, block, 0, c->stream, c->d_raw.as<const uint8_t>(), w, h, stride, 0, (const int16_t *)c->map_xy, (const uint16_t *)c->map_frac, npix, g0, c->d_col.as<uint8_t>());
        else hipLaunchKernelGGL((k_undist_grey<1, false>), grid, block, 0, c->stream, c->d_raw.as<const uint8_t>(), w, h, stride, 0, (const int16_t *)c->map_xy, (const uint16_t *)c->map_frac, npix, g0, (uint8_t *)nullptr);
    }
    if (undist_out) CKF(hipMemcpyAsync(c->h_stage.as(), c->d_col.as(), col_bytes, hipMemcpyDeviceToHost, c->stream));      // (the raw frame has left the staging: same stream)
    rc = pyramid_from_level0(c); if (rc) return rc;
    if (undist_out) memcpy(undist_out, c->h_stage.as(), col_bytes);
    return TSFRAME_OK;
}
int tsframe_level_size(void *ctx, int level, int *w, int *h) {
    FCtx *c = (FCtx *)ctx; if (!c || level < 0 || level >= c->n_levels) return TSFRAME_ERR_ARG;
    if (w) *w = c->w[level];
    if (h) *h = c->h[level];
    return TSFRAME_OK;
}
int tsframe_level_ptr(void *ctx, int level, int which, const uint8_t **dev) {
    FCtx *c = (FCtx *)ctx; if (!c || !dev || level < 0 || level >= c->n_levels || which < 0 || which > 3) return TSFRAME_ERR_ARG;
    *dev = c->plane[which][level]; return TSFRAME_OK;
}
int tsframe_get_level(void *ctx, int level, int which, uint8_t *out) {
    FCtx *c = (FCtx *)ctx; if (!c || !out || level < 0 || level >= c->n_levels || which < 0 || which > 3) return TSFRAME_ERR_ARG;
    hipSetDevice(c->device);
    CKF(hipMemcpy(out, c->plane[which][level], (size_t)c->w[level]*c->h[level], hipMemcpyDeviceToHost));
    return TSFRAME_OK;
}

int tsframe_pyramid_pts(void *ctx, int mode, const float *xy, int n, const double *box, const double *inv_scale,
                        int32_t *level_off, double *u, double *v, int32_t *idx, double *inten, uint8_t *in) {
    FCtx *c = (FCtx *)ctx;
    if (!c || n < 0 || (n > 0 && !xy) || !inv_scale || !level_off || !u || !v || !idx || !inten || !in || (mode != 0 && mode != 1) || (mode == 0 && !box)) return TSFRAME_ERR_ARG;
    if (c->n_levels == 0) { c->err = "no image set"; return TSFRAME_ERR_STATE; }
    if (n > INT32_MAX / c->n_levels) { c->err = "more than INT32_MAX / n_levels features"; return TSFRAME_ERR_ARG; }
    // the batch of one set
    const int32_t xy_off[2] = { 0, n };
    std::vector<PtsJob> jobs((size_t)c->n_levels);
    size_t sel_ints = 0;
    if (const char *why = pts_set_jobs(c, mode, 0, n, box, inv_scale, jobs.data(), sel_ints)) { c->err = why; return TSFRAME_ERR_ARG; }
    return pts_run(c, 1, xy_off, xy, jobs, sel_ints, level_off, u, v, idx, inten, in);
}

int tsframe_pyramid_pts_batch(void *ctx, int n_set, const int32_t *mode, const int32_t *xy_off, const float *xy, const double *box, const double *inv_scale,
                              int32_t *level_off, double *u, double *v, int32_t *idx, double *inten, uint8_t *in) {
    FCtx *c = (FCtx *)ctx;
    if (!c) return TSFRAME_ERR_ARG;
    auto bad = [&](const std::string &what) { c->err = "tsframe_pyramid_pts_batch: " + what; return TSFRAME_ERR_ARG; };
    auto at_set = [](const char *what, int i) { return std::string(what) + " (set " + std::to_string(i) + ")"; };
    if (n_set < 0) return bad("n_set < 0");
    if (n_set == 0) return TSFRAME_OK;
    if (!mode || !xy_off || !inv_scale || !level_off) return bad("NULL mode / xy_off / inv_scale / level_off");
    if (c->n_levels == 0) { c->err = "tsframe_pyramid_pts_batch: no image set"; return TSFRAME_ERR_STATE; }
    const int L = c->n_levels;
    const double lim = 1048576.0;                                // 2^20: keeps the cell index inside an int, here and in the CPU restatement
    auto wild = [lim](double x) { return !(fabs(x) <= lim); };   // (NaN and infinities included)
    for (int l = 0; l < L; l++) if (wild(inv_scale[l])) return bad("inv_scale not finite or above 2^20 in magnitude");
    if (xy_off[0] != 0) return bad("xy_off[0] != 0");
    bool any_text = false;
    for (int i = 0; i < n_set; i++) {
        if (mode[i] != 0 && mode[i] != 1) return bad(at_set("mode is neither 0 nor 1", i));
        if (xy_off[i + 1] < xy_off[i]) return bad(at_set("xy_off decreasing", i));
        any_text |= mode[i] == 0;
    }
    const size_t total = (size_t)xy_off[n_set];
    if (total > (size_t)(INT32_MAX / L)) return bad("more than INT32_MAX / n_levels features");
    if (any_text && !box) return bad("box NULL with a text set");
    if (total > 0 && (!xy || !u || !v || !idx || !inten || !in)) return bad("NULL array with features");
    for (size_t k = 0; k < 2*total; k++)
        if (wild((double)xy[k])) {
            int i = 0; while (xy_off[i + 1] <= (int32_t)(k/2)) i++;
            return bad(at_set("coordinate not finite or above 2^20 in magnitude", i));
        }
    // a set's box, then its jobs: a refusal names the first set that has either fault
    std::vector<PtsJob> jobs((size_t)n_set*L);
    size_t sel_ints = 0;
    for (int i = 0; i < n_set; i++) {
        const double *bx = mode[i] == 0 ? box + 4*(size_t)i : nullptr;
        if (bx) for (int k = 0; k < 4; k++) if (wild(bx[k])) return bad(at_set("box not finite or above 2^20 in magnitude", i));
        if (const char *why = pts_set_jobs(c, mode[i], xy_off[i], xy_off[i + 1] - xy_off[i], bx, inv_scale, &jobs[(size_t)i*L], sel_ints)) return bad(at_set(why, i));
    }
    return pts_run(c, n_set, xy_off, xy, jobs, sel_ints, level_off, u, v, idx, inten, in);
}

int tsframe_neighbours(void *ctx, int level, const double *uv, int n, double mu, double sigma, double *inten8, double *ninten8, uint8_t *in) {
    FCtx *c = (FCtx *)ctx;
    if (!c || n < 0 || (n > 0 && (!uv || !inten8 || !ninten8 || !in)) || level < 0) return TSFRAME_ERR_ARG;
    if (level >= c->n_levels) { c->err = "level not built"; return TSFRAME_ERR_STATE; }
    if (sigma == 0.0) { c->err = "sigma == 0 (tool::CalNormvec returns false)"; return TSFRAME_ERR_ARG; }
    if (n == 0) return TSFRAME_OK;
    hipSetDevice(c->device);
    // one block: uv || inten8 | ninten8 | in
    Layout L(256);
    const auto a_uv = L.take<double>(2*(size_t)n);
    const auto a_I = L.take<double>(8*(size_t)n), a_N = L.take<double>(8*(size_t)n); const auto a_in = L.take<uint8_t>((size_t)n);
    CKF(c->d_work.grow(L.mark())); CKF(c->h_stage.grow(L.mark()));
    void *h = c->h_stage.as(), *d = c->d_work.as();
    a_uv.put(h, uv);
    CKF(hipMemcpyAsync(d, h, a_uv.bytes(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_neighbours, dim3((8*n + 255)/256), dim3(256), 0, c->stream, (const uint8_t *)c->plane[TSFRAME_IMG][level], c->w[level], c->h[level],
                       a_uv.at(d), n, mu, sigma, a_I.at(d), a_N.at(d), a_in.at(d));
    CKF(hipMemcpyAsync(a_I.at(h), a_I.at(d), L.mark() - a_I.off, hipMemcpyDeviceToHost, c->stream));
    CKF(hipStreamSynchronize(c->stream)); CKF(hipGetLastError());
    a_I.get(h, inten8); a_N.get(h, ninten8); a_in.get(h, in);
    return TSFRAME_OK;
}

int tsframe_box_pixels(void *ctx, int level, const double *quad, double mu, double sigma, int cap, int32_t *n_out,
                       int32_t *u, int32_t *v, double *inten, double *ninten) {
    FCtx *c = (FCtx *)ctx;
    if (!c || !quad || !n_out || cap < 0 || (cap > 0 && (!u || !v || !inten || !ninten)) || level < 0) return TSFRAME_ERR_ARG;
    if (level >= c->n_levels) { c->err = "level not built"; return TSFRAME_ERR_STATE; }
    for (int i = 0; i < 8; i++) if (!(fabs(quad[i]) < 1e9)) { c->err = "quad corner not finite"; return TSFRAME_ERR_ARG; }
    hipSetDevice(c->device);
    const int w = c->w[level], h = c->h[level];
    BoxDev B;
    quad_box(quad, 1.0, w, h, B.xy, B.x0, B.x1, B.y0, B.y1);
    const int xMin = B.x0, xMax = B.x1, yMin = B.y0, yMax = B.y1;
    *n_out = 0;
    if (xMax < xMin || yMax < yMin) return TSFRAME_OK;
    const size_t npx = (size_t)(xMax - xMin + 1)*(size_t)(yMax - yMin + 1);
    // one block, outputs only: cnt | mask (the kernel's scratch) | u | v | inten | ninten, the four arrays with room for the whole box
    Layout L(256);
    const auto a_cnt = L.take<int32_t>(1); const auto a_mask = L.take<unsigned>(((size_t)w*h + 31) >> 5);
    const auto a_u = L.take<int32_t>(npx), a_v = L.take<int32_t>(npx); const auto a_I = L.take<double>(npx), a_N = L.take<double>(npx);
    CKF(c->d_work.grow(L.mark())); CKF(c->h_stage.grow(L.mark()));
    void *hs = c->h_stage.as(), *d = c->d_work.as();
    hipLaunchKernelGGL(k_box_pixels, dim3(1), dim3(1024), 0, c->stream, (const uint8_t *)c->plane[TSFRAME_IMG][level], w, h, B, mu, sigma, a_mask.at(d),
                       a_cnt.at(d), a_u.at(d), a_v.at(d), a_I.at(d), a_N.at(d));
    CKF(hipMemcpyAsync(a_cnt.at(hs), a_cnt.at(d), a_cnt.bytes(), hipMemcpyDeviceToHost, c->stream));
    CKF(hipStreamSynchronize(c->stream)); CKF(hipGetLastError());
    const int n = *a_cnt.at(hs);
    *n_out = n;
    if (cap == 0 || n == 0) return TSFRAME_OK;                      // cap == 0: count only
    if (n > cap) { c->err = "tsframe_box_pixels: capacity too small (n_out holds the count)"; return TSFRAME_ERR_ARG; }
    // the first n entries of each array come down: the same offsets, n elements
    const Span<int32_t> g_u{a_u.off, (size_t)n}, g_v{a_v.off, (size_t)n}; const Span<double> g_I{a_I.off, (size_t)n}, g_N{a_N.off, (size_t)n};
    CKF(hipMemcpyAsync(g_u.at(hs), g_u.at(d), g_u.bytes(), hipMemcpyDeviceToHost, c->stream));
    CKF(hipMemcpyAsync(g_v.at(hs), g_v.at(d), g_v.bytes(), hipMemcpyDeviceToHost, c->stream));
    CKF(hipMemcpyAsync(g_I.at(hs), g_I.at(d), g_I.bytes(), hipMemcpyDeviceToHost, c->stream));
    CKF(hipMemcpyAsync(g_N.at(hs), g_N.at(d), g_N.bytes(), hipMemcpyDeviceToHost, c->stream));
    CKF(hipStreamSynchronize(c->stream));
    g_u.get(hs, u); g_v.get(hs, v); g_I.get(hs, inten); g_N.get(hs, ninten);
    return TSFRAME_OK;
}

int tsframe_text_judge(void *ctx, int level, int n, const double *theta, const double *Tcr, const double *box_ray,
                       const int32_t *pix_off, const int16_t *pix_uv, const uint8_t *pix_inten,
                       const double K_ref[4], const double K[4], double cos_min, int out_margin, double zncc_min,
                       int n_dete, const double *dete_xy,
                       uint8_t *pass, int32_t *reason, double *cos, double *zncc, double *box_uv, uint32_t *dete_bits) {
    FCtx *c = (FCtx *)ctx;
    if (!c) return TSFRAME_ERR_ARG;
    auto bad = [&](const char *what) { c->err = std::string("tsframe_text_judge: ") + what; return TSFRAME_ERR_ARG; };
    if (n < 0) return bad("n < 0");
    if (level < 0) return bad("level < 0");
    if (n_dete < 0 || (n_dete > 0 && !dete_xy)) return bad("n_dete < 0, or dete_xy NULL with n_dete > 0");
    if (out_margin < 0) return bad("out_margin < 0");
    if (n == 0) return TSFRAME_OK;
    if (!theta || !Tcr || !box_ray || !pix_off || !K_ref || !K || !pass || !reason || !cos || !zncc || !box_uv) return bad("NULL array");
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(K_ref[k]) || !std::isfinite(K[k]) || (k < 2 && (K_ref[k] == 0.0 || K[k] == 0.0))) return bad("K_ref / K not finite or zero focal length");
    if (pix_off[0] != 0) return bad("pix_off[0] != 0");
    for (int i = 0; i < n; i++) if (pix_off[i + 1] < pix_off[i]) return bad("pix_off decreasing");
    const size_t npix = (size_t)pix_off[n];
    if (npix > 0 && (!pix_uv || !pix_inten)) return bad("pix_uv / pix_inten NULL with pixels");
    if (c->n_levels == 0) { c->err = "tsframe_text_judge: no image set"; return TSFRAME_ERR_STATE; }
    if (level >= c->n_levels) { c->err = "tsframe_text_judge: level not built"; return TSFRAME_ERR_STATE; }
    const int words = dete_bits ? (n_dete + 31)/32 : 0;
    hipSetDevice(c->device);
    JudgeArgs A;
    A.w = c->w[level]; A.h = c->h[level]; A.w0 = c->w[0]; A.h0 = c->h[0]; A.margin = out_margin; A.n_dete = n_dete; A.dete_words = words;
    for (int k = 0; k < 4; k++) { A.Kr[k] = K_ref[k]; A.K[k] = K[k]; }
    A.cos_min = cos_min; A.zncc_min = zncc_min;
    // one pinned block, inputs then outputs: planes | dete_xy | pix_off | pix_uv | pix_inten || out | bits
    const size_t nd = words > 0 ? (size_t)n_dete : 0;
    Layout L(256);
    const auto a_pl = L.take<JudgePlane>((size_t)n); const auto a_dx = L.take<double>(2*nd); const auto a_off = L.take<int32_t>((size_t)n + 1);
    const auto a_uv = L.take<int16_t>(2*npix); const auto a_in = L.take<uint8_t>(npix);
    const size_t in_end = L.mark();
    const auto a_out = L.take<JudgeOut>((size_t)n); const auto a_bits = L.take<uint32_t>((size_t)n*words);
    CKF(c->d_work.grow(L.mark())); CKF(c->h_stage.grow(L.mark()));
    void *h = c->h_stage.as(), *d = c->d_work.as();
    JudgePlane *hp = a_pl.at(h);
    for (int i = 0; i < n; i++) {
        std::copy_n(theta + 3*(size_t)i, 3, hp[i].theta); std::copy_n(Tcr + 12*(size_t)i, 12, hp[i].T); std::copy_n(box_ray + 8*(size_t)i, 8, hp[i].ray);
    }
    a_dx.put(h, dete_xy); a_off.put(h, pix_off); a_uv.put(h, pix_uv); a_in.put(h, pix_inten);
    CKF(hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, c->stream));
    if (words > 0 && (size_t)c->w[0]*c->h[0] > (size_t)MS_MASK_WORDS*32)       // the association's mask is level-0 sized: above it, point tests instead
        hipLaunchKernelGGL(k_text_judge<true>, dim3(n), dim3(JUDGE_NT), 0, c->stream, (const uint8_t *)c->plane[TSFRAME_IMG][level], A, a_pl.at(d),
                           a_off.at(d), a_uv.at(d), a_in.at(d), a_dx.at(d), a_out.at(d), a_bits.at(d));
    else
        hipLaunchKernelGGL(k_text_judge<false>, dim3(n), dim3(JUDGE_NT), 0, c->stream, (const uint8_t *)c->plane[TSFRAME_IMG][level], A, a_pl.at(d),
                           a_off.at(d), a_uv.at(d), a_in.at(d), a_dx.at(d), a_out.at(d), words > 0 ? a_bits.at(d) : nullptr);
    CKF(hipGetLastError());
    CKF(hipMemcpyAsync(a_out.at(h), a_out.at(d), L.mark() - in_end, hipMemcpyDeviceToHost, c->stream));
    CKF(hipStreamSynchronize(c->stream));
    const JudgeOut *ho = a_out.at(h);
    for (int i = 0; i < n; i++) {
        reason[i] = ho[i].reason; pass[i] = ho[i].reason == TSFRAME_JUDGE_PASS ? 1 : 0; cos[i] = ho[i].cos; zncc[i] = ho[i].zncc;
        std::copy_n(ho[i].box, 8, box_uv + 8*(size_t)i);
    }
    a_bits.get(h, dete_bits);
    return TSFRAME_OK;
}

int tsframe_klt_track(void *prev_ctx, void *cur_ctx, int n, const float *prev_xy, int win, int max_level, int max_iter, double eps, double min_eig,
                      float *next_xy, uint8_t *status) {
    FCtx *p = (FCtx *)prev_ctx, *c = (FCtx *)cur_ctx;
    if (!c) return TSFRAME_ERR_ARG;
    auto bad = [&](const char *what) { c->err = std::string("tsframe_klt_track: ") + what; return TSFRAME_ERR_ARG; };
    if (!p) return bad("prev_ctx NULL");
    if (n < 0) return bad("n < 0");
    if (n > 0 && (!prev_xy || !next_xy || !status)) return bad("NULL array with n > 0");
    if (win < 3 || win > 31 || !(win & 1)) return bad("win must be odd and in [3, 31]");
    if (max_level < 0 || max_level > TSFRAME_MAX_LEVELS - 1) return bad("max_level outside [0, 7]");
    if (max_iter < 1 || max_iter > 100) return bad("max_iter outside [1, 100]");
    if (!(eps >= 0.0)) return bad("eps < 0");
    if (n == 0) return TSFRAME_OK;
    if (p->n_levels == 0 || c->n_levels == 0) { c->err = "tsframe_klt_track: no image set"; return TSFRAME_ERR_STATE; }
    if (p->device != c->device) return bad("the two contexts are on different devices");
    if (p->w[0] != c->w[0] || p->h[0] != c->h[0]) return bad("the level-0 sizes differ");
    // the level rule: L + 1 levels, L <= max_level; level l and all coarser ones are dropped if its width or height is <= win
    if (c->w[0] <= win || c->h[0] <= win) return bad("the level-0 image must be larger than the window");
    int need = 1, lw = c->w[0], lh = c->h[0];
    for (int l = 1; l <= max_level; l++) { lw = (lw + 1)/2; lh = (lh + 1)/2; if (lw <= win || lh <= win) break; need = l + 1; }
    if (p->n_levels < need || c->n_levels < need) return bad("a context holds fewer resident levels than max_level and the image size ask for");
    hipSetDevice(c->device);
    KltArgs A;
    for (int l = 0; l < TSFRAME_MAX_LEVELS; l++) {
        const bool on = l < need;
        A.I[l] = on ? p->plane[TSFRAME_IMG][l] : nullptr; A.J[l] = on ? c->plane[TSFRAME_IMG][l] : nullptr; A.w[l] = on ? c->w[l] : 0; A.h[l] = on ? c->h[l] : 0;
    }
    A.n = n; A.n_levels = need; A.win = win; A.max_iter = max_iter;
    A.eps2 = (float)eps*(float)eps; A.min_eig = (float)min_eig;
    // one pinned block: prev_xy || next_xy | status
    Layout L(256);
    const auto a_prev = L.take<float>(2*(size_t)n);
    const auto a_next = L.take<float>(2*(size_t)n); const auto a_st = L.take<uint8_t>((size_t)n);
    CKF(c->d_work.grow(L.mark())); CKF(c->h_stage.grow(L.mark()));
    void *h = c->h_stage.as(), *d = c->d_work.as();
    a_prev.put(h, prev_xy);
    CKF(hipMemcpyAsync(d, h, a_prev.bytes(), hipMemcpyHostToDevice, c->stream));
    const dim3 grid((n + KLT_WAVES - 1)/KLT_WAVES), block(64*KLT_WAVES);
    if (win*win <= 64*8) hipLaunchKernelGGL(k_klt_track<8>, grid, block, 0, c->stream, A, a_prev.at(d), a_next.at(d), a_st.at(d));
    else hipLaunchKernelGGL(k_klt_track<16>, grid, block, 0, c->stream, A, a_prev.at(d), a_next.at(d), a_st.at(d));
    CKF(hipGetLastError());
    CKF(hipMemcpyAsync(a_next.at(h), a_next.at(d), L.mark() - a_next.off, hipMemcpyDeviceToHost, c->stream));
    CKF(hipStreamSynchronize(c->stream));
    a_next.get(h, next_xy); a_st.get(h, status);
    return TSFRAME_OK;
}

int tsframe_text_object_info(void *ctx, int n_obj, const double *quad, const double *inv_scale, const int32_t *feat_off, const int32_t *level_off,
                             const double *u, const double *v, const double *inten, int pix_cap,
                             double *musigma, uint8_t *ok, double *ninten, double *inten8, double *ninten8, uint8_t *in,
                             int32_t *pix_off, int32_t *pix_u, int32_t *pix_v, double *pix_inten, double *pix_ninten) {
    FCtx *c = (FCtx *)ctx;
    if (!c) return TSFRAME_ERR_ARG;
    auto bad = [&](const std::string &what) { c->err = "tsframe_text_object_info: " + what; return TSFRAME_ERR_ARG; };
    auto at_obj = [](const char *what, int i) { return std::string(what) + " (object " + std::to_string(i) + ")"; };
    if (n_obj < 0) return bad("n_obj < 0");
    if (n_obj == 0) return TSFRAME_OK;
    if (!quad || !inv_scale || !feat_off || !level_off || !musigma || !ok || !pix_off) return bad("NULL quad / inv_scale / feat_off / level_off / musigma / ok / pix_off");
    if (pix_cap < 0) return bad("pix_cap < 0");
    if (pix_cap > 0 && (!pix_u || !pix_v || !pix_inten || !pix_ninten)) return bad("NULL pixel array with pix_cap > 0");
    if (c->n_levels == 0) { c->err = "tsframe_text_object_info: no image set"; return TSFRAME_ERR_STATE; }
    const int L = c->n_levels;
    if ((size_t)c->w[0] > (size_t)MS_MASK_WORDS*32) return bad("the image is wider than one band of the quad mask");
    auto wild = [](double x) { return !(fabs(x) < 1e9); };       // (NaN and infinities included)
    for (int l = 0; l < L; l++) if (wild(inv_scale[l])) return bad("inv_scale not finite or >= 1e9 in magnitude");
    if (feat_off[0] != 0) return bad("feat_off[0] != 0");
    size_t nfeat = 0;                                            // the packed features: object i's [0, level_off[i][L]) only
    for (int i = 0; i < n_obj; i++) {
        if (feat_off[i + 1] < feat_off[i]) return bad(at_obj("feat_off decreasing", i));
        const int32_t *lo = level_off + (size_t)i*(L + 1);
        if (lo[0] != 0) return bad(at_obj("level_off row does not start at 0", i));
        for (int l = 0; l < L; l++) if (lo[l + 1] < lo[l]) return bad(at_obj("level_off decreasing", i));
        if ((long long)lo[L] > (long long)(feat_off[i + 1] - feat_off[i])*L) return bad(at_obj("level_off ends above the object's slice", i));
        for (int k = 0; k < 8; k++) {
            if (wild(quad[8*(size_t)i + k])) return bad(at_obj("corner not finite or >= 1e9 in magnitude", i));
            for (int l = 0; l < L; l++) if (wild(quad[8*(size_t)i + k]*inv_scale[l])) return bad(at_obj("scaled corner >= 1e9 in magnitude", i));
        }
        nfeat += (size_t)lo[L];
    }
    if ((size_t)feat_off[n_obj] > (size_t)(INT32_MAX / L) || nfeat > (size_t)(INT32_MAX / 8)) return bad("too many features");
    if (nfeat > 0 && (!u || !v || !inten || !ninten || !inten8 || !ninten8 || !in)) return bad("NULL feature array with features");
    for (int i = 0; i < n_obj; i++) {
        const size_t b = (size_t)feat_off[i]*L, m = (size_t)level_off[(size_t)i*(L + 1) + L];
        for (size_t k = b; k < b + m; k++) if (!std::isfinite(u[k]) || !std::isfinite(v[k])) return bad(at_obj("u / v not finite", i));
    }
    // jobs: one per (object, level); the corners are quad * inv_scale[l] (mapText.cc:78-81), truncated and boxed by quad_box
    std::vector<ObjJob> jobs((size_t)n_obj*L);
    std::vector<size_t> fbase((size_t)n_obj + 1, 0), pbase((size_t)n_obj + 1, 0);
    const bool want_pix = pix_cap > 0;
    for (int i = 0; i < n_obj; i++) {
        const int32_t *lo = level_off + (size_t)i*(L + 1);
        for (int l = 0; l < L; l++) {
            ObjJob &J = jobs[(size_t)i*L + l];
            const int w = c->w[l], h = c->h[l];
            quad_box(quad + 8*(size_t)i, inv_scale[l], w, h, J.xy, J.x0, J.x1, J.y0, J.y1);
            const int xMin = J.x0, xMax = J.x1, yMin = J.y0, yMax = J.y1;
            J.img = c->plane[TSFRAME_IMG][l]; J.w = w; J.h = h;
            J.f0 = (int)(fbase[i] + (size_t)lo[l]); J.nf = lo[l + 1] - lo[l];
            J.pix0 = -1;
            if (l == 0) {
                const size_t area = (xMax >= xMin && yMax >= yMin) ? (size_t)(xMax - xMin + 1)*(size_t)(yMax - yMin + 1) : 0;
                if (want_pix) J.pix0 = (long long)pbase[i];
                pbase[i + 1] = pbase[i] + area;
            }
        }
        fbase[i + 1] = fbase[i] + (size_t)lo[L];
    }
    const size_t nreg = want_pix ? pbase[n_obj] : 0;             // slots of the pixel regions (the sum of the clamped level-0 boxes)
    hipSetDevice(c->device);
    // one block, inputs then outputs: jobs | u | v | inten || out | ninten | inten8 | ninten8 | in | pix_u | pix_v | pix_inten | pix_ninten
    Layout S(256);
    const auto a_job = S.take<ObjJob>(jobs.size()); const auto a_u = S.take<double>(nfeat), a_v = S.take<double>(nfeat), a_I = S.take<double>(nfeat);
    const size_t in_end = S.mark();
    const auto a_out = S.take<ObjOut>(jobs.size()); const auto a_n = S.take<double>(nfeat), a_i8 = S.take<double>(8*nfeat), a_n8 = S.take<double>(8*nfeat);
    const auto a_in = S.take<uint8_t>(nfeat);
    const size_t feat_end = S.mark();                            // a count-only call's copy down ends here
    const auto a_pu = S.take<int32_t>(nreg), a_pv = S.take<int32_t>(nreg); const auto a_pI = S.take<double>(nreg), a_pN = S.take<double>(nreg);
    CKF(c->d_work.grow(S.mark())); CKF(c->h_stage.grow(S.mark()));
    void *h = c->h_stage.as(), *d = c->d_work.as();
    a_job.put(h, jobs.data());
    for (int i = 0; i < n_obj; i++) {
        const size_t b = (size_t)feat_off[i]*L, m = fbase[i + 1] - fbase[i];
        if (!m) continue;
        std::copy_n(u + b, m, a_u.at(h) + fbase[i]); std::copy_n(v + b, m, a_v.at(h) + fbase[i]); std::copy_n(inten + b, m, a_I.at(h) + fbase[i]);
    }
    CKF(hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_object_info, dim3((unsigned)a_job.n), dim3(OBJ_NT), 0, c->stream, a_job.at(d), a_u.at(d), a_v.at(d), a_I.at(d),
                       a_out.at(d), a_n.at(d), a_i8.at(d), a_n8.at(d), a_in.at(d), a_pu.at(d), a_pv.at(d), a_pI.at(d), a_pN.at(d));
    CKF(hipGetLastError());
    CKF(hipMemcpyAsync(a_out.at(h), a_out.at(d), (want_pix ? S.mark() : feat_end) - in_end, hipMemcpyDeviceToHost, c->stream));
    CKF(hipStreamSynchronize(c->stream));
    const ObjOut *ho = a_out.at(h);
    long long total = 0;
    pix_off[0] = 0;
    for (int i = 0; i < n_obj; i++) {
        for (int l = 0; l < L; l++) {
            const ObjOut &o = ho[(size_t)i*L + l];
            musigma[2*((size_t)i*L + l)] = o.mu; musigma[2*((size_t)i*L + l) + 1] = o.sigma; ok[(size_t)i*L + l] = (uint8_t)o.ok;
        }
        const size_t b = (size_t)feat_off[i]*L, m = fbase[i + 1] - fbase[i];
        if (m) {
            std::copy_n(a_n.at(h) + fbase[i], m, ninten + b); std::copy_n(a_i8.at(h) + 8*fbase[i], 8*m, inten8 + 8*b);          // (8 taps per feature)
            std::copy_n(a_n8.at(h) + 8*fbase[i], 8*m, ninten8 + 8*b); std::copy_n(a_in.at(h) + fbase[i], m, in + b);
        }
        total += std::min((long long)ho[(size_t)i*L].npix, (long long)(pbase[i + 1] - pbase[i]));
        pix_off[i + 1] = (int32_t)std::min(total, (long long)INT32_MAX);
    }
    if (pix_cap == 0) return TSFRAME_OK;                         // count only
    if (total > (long long)pix_cap) return bad("pix_cap too small (pix_off holds the counts)");
    for (int i = 0; i < n_obj; i++) {                            // close the gaps between the regions
        const size_t src = pbase[i], dst = (size_t)pix_off[i], m = (size_t)(pix_off[i + 1] - pix_off[i]);
        if (!m) continue;
        std::copy_n(a_pu.at(h) + src, m, pix_u + dst); std::copy_n(a_pv.at(h) + src, m, pix_v + dst);
        std::copy_n(a_pI.at(h) + src, m, pix_inten + dst); std::copy_n(a_pN.at(h) + src, m, pix_ninten + dst);
    }
    return TSFRAME_OK;
}

}  // extern "C"
