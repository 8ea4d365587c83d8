// tscvorb.h -- frame::FeatExtracText (src/frame.cc:334-355) on the device: cv::ORB::create()->detect on the frame masked to each text
// detection's quad (tool::GetMask) and ->compute on the frame itself, for all detections of a frame in one call.  docs/cvorb_recalled.md is the
// arithmetic (OpenCV 3.3 defaults); included by tsorb.hip behind resize_xent / resize_yent / fast_score / fast_atan2f_dev / d_pattern.
//
// The launches of a call, whatever the number of detections (grids span detection x level x tile):
//   k_cvo_mask      one workgroup per detection: cv::fillPoly of the quad (raster_quad) -> the detection's bit mask
//   k_cvo_resize    x 7, level l from level l-1: plane 0 of the grid is the unmasked cv::ORB pyramid (once per call), plane 1 + d the masked
//                   pyramid of detection d, restricted to the detection's footprint at that level
//   k_cvo_blur      the unmasked levels' 7x7 Gaussian (once per call)
//   k_cvo_fast      whole-level FAST-9/16 at 20 + strict 3x3 suppression + the 31-px border rule, a 32 x 32 tile per workgroup -> per-tile lists
//   k_cvo_select    one workgroup per (detection, level): score histogram -> first cut, Harris responses of its survivors, radix select on the
//                   fp32 response -> second cut, the survivors per level row and their exclusive scan
//   k_cvo_place     a survivor's place = the levels before + the rows before + the survivors of its row to its left: level-major raster order
//   k_cvo_describe  32 lanes per keypoint: IC_Angle on the masked level, steered BRIEF on the blurred unmasked level, the six keypoint fields
// A masked image is zero outside its quad, so level l of it is zero outside a rectangle (the footprint: the quad's bounding box taken through the
// resize supports, formed on the host with a margin).  Only the footprint is stored; every read of a masked level goes through cvo_m, which
// answers 0 outside it -- the bytes of the whole level.  No workgroup waits for another; every loop is bounded by a constant of this file or by
// a size of the geometry; every read is inside a footprint, clamped or reflected.
#pragma once
#include "tsraster.h"

#define CVO_NL 8
#define CVO_MAX_W 640
#define CVO_MAX_H 480
#define CVO_TS 32                       // FAST tile (output pixels per side)
#define CVO_TCAP 256                    // corners a tile can hold after the strict 3 x 3 suppression: one per 2 x 2 pixels
#define CVO_MAX_T ((CVO_MAX_W/CVO_TS)*(CVO_MAX_H/CVO_TS))      // tiles of the largest level
#define CVO_BORDER 31                   // edgeThreshold
#define CVO_DESC_BLOCKS 64

struct CvoLevel {
    int w, h, ntx, nty, tile0, quota;
    int xt_off, yt_off;                 // cv::resize tables of this level (from level l-1) inside CvoDev::rtab
    size_t off, boff;                   // byte offset of the level inside a pyramid slab (levels 1 ..; level 0 is the resident frame) / the blur slab
    float scale, inv;                   // (float)pow(1.2f, l), 1.f / that
    double rsx, rsy;
};
struct CvoDev {
    int w, h, nd, cap, ntiles;
    CvoLevel L[CVO_NL];
    const uint8_t *img0; int pitch0;    // level 0 of the resident frame: the interior of the bordered plane k_level0 wrote
    uint8_t *U, *B, *M; size_t m_stride;        // unmasked pyramid, its blurred copy, masked pyramids [nd][m_stride]
    int *rtab;
    unsigned *mask;                     // [nd][MS_MASK_WORDS]
    const int *quad, *foot;             // (pinned) [nd][8] truncated corners, [nd][CVO_NL][4] footprint x0, y0, x1, y1 (empty: x0 > x1)
    int *dfoot;                         // the footprints in device memory (k_cvo_mask copies them: every workgroup of every later launch reads one)
    uint32_t *tkp, *tkey; int *tcnt;    // [nd][ntiles][CVO_TCAP] x | y << 10 | score << 20, the response's ordered key; [nd][ntiles]
    int *rowoff, *lvlcnt; uint32_t *thr;        // [nd][CVO_NL][CVO_MAX_H], [nd][CVO_NL], [nd][CVO_NL][2] first cut (score), second cut (key)
    float4 *sel;                        // [nd][cap] x, y (level coordinates), response, level
    int *o_cnt; float *o_kp; uint8_t *o_desc;   // [nd], [nd][cap][6], [nd][cap][32]: the pinned block (tsorb_text_extract) or device scratch (tsorb_fuse_frame)
    int umax[16], gk[7];
};

__device__ __forceinline__ int4 cvo_foot(const CvoDev &C, int d, int l) { return ((const int4 *)C.dfoot)[(size_t)d*CVO_NL + l]; }
// pixel (x, y) of level l of detection d's masked pyramid; R = cvo_foot(C, d, l).  Any x, y: 0 outside the footprint (which lies inside the level)
__device__ __forceinline__ int cvo_m(const CvoDev &C, int d, int l, const int4 R, int x, int y) {
    if (x < R.x || x > R.z || y < R.y || y > R.w) return 0;
    if (l == 0) { const int bit = y*C.w + x; return ((C.mask[(size_t)d*MS_MASK_WORDS + (bit >> 5)] >> (bit & 31)) & 1u) ? C.img0[(size_t)y*C.pitch0 + x] : 0; }
    return C.M[(size_t)d*C.m_stride + C.L[l].off + (size_t)y*C.L[l].w + x];
}
__device__ __forceinline__ void cvo_tile(const CvoDev &C, int t, int &l, int &tx, int &ty) {
    l = 0;
#pragma unroll
    for (int k = 1; k < CVO_NL; k++) if (t >= C.L[k].tile0) l = k;
    const int r = t - C.L[l].tile0; ty = r / C.L[l].ntx; tx = r - ty*C.L[l].ntx;
}
// fp32 -> a key whose unsigned order is the order of the values; -0.f and +0.f share a key (OpenCV's comparator calls them equal)
__device__ __forceinline__ uint32_t cvo_key(float v) { const uint32_t b = __float_as_uint(__fadd_rn(v, 0.f)); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float cvo_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void k_cvo_tab(CvoDev C) {             // once per geometry
    const int l = blockIdx.x + 1;
    const CvoLevel &G = C.L[l], &S = C.L[l-1];
    int2 *xt = (int2 *)(C.rtab + G.xt_off); int4 *yt = (int4 *)(C.rtab + G.yt_off);
    for (int x = threadIdx.x; x < G.w; x += 256) xt[x] = resize_xent(x, G.rsx, S.w);
    for (int y = threadIdx.x; y < G.h; y += 256) yt[y] = resize_yent(y, G.rsy, S.h);
}

__global__ __launch_bounds__(256) void k_cvo_mask(CvoDev C) {
    __shared__ unsigned mask[MS_MASK_WORDS];
    __shared__ int s_xy[8];
    const int d = blockIdx.x, tid = threadIdx.x, nw = (C.w*C.h + 31) >> 5;        // (w h <= 640 x 480: nw <= MS_MASK_WORDS)
    for (int k = tid; k < nw; k += 256) mask[k] = 0;
    if (tid < 8) s_xy[tid] = C.quad[8*d + tid];
    if (tid < 4*CVO_NL) C.dfoot[4*CVO_NL*d + tid] = C.foot[4*CVO_NL*d + tid];
    __syncthreads();
    raster_quad(mask, s_xy, C.w, C.h, tid, 256);
    __syncthreads();
    for (int k = tid; k < nw; k += 256) C.mask[(size_t)d*MS_MASK_WORDS + k] = mask[k];
}

// cv::resize INTER_LINEAR (V4) of level l from level l-1.  grid (64-px column chunks, groups of 4 rows, 1 + nd)
__global__ __launch_bounds__(256) void k_cvo_resize(CvoDev C, int l) {
    const CvoLevel &G = C.L[l], &S = C.L[l-1];
    const int x = blockIdx.x*64 + (threadIdx.x & 63), y = blockIdx.y*4 + (threadIdx.x >> 6), z = blockIdx.z;
    if (x >= G.w || y >= G.h) return;
    int4 R = make_int4(0, 0, 0, 0), RS = R;
    if (z > 0) { R = cvo_foot(C, z - 1, l); if (x < R.x || x > R.z || y < R.y || y > R.w) return; RS = cvo_foot(C, z - 1, l - 1); }
    const int2 xe = ((const int2 *)(C.rtab + G.xt_off))[x]; const int4 ye = ((const int4 *)(C.rtab + G.yt_off))[y];
    const int sx = xe.x & 0xffff, sx1 = xe.x >> 16, a0 = xe.y & 0xffff, a1 = xe.y >> 16;       // (all inside level l-1: the tables clamp)
    int p00, p01, p10, p11; uint8_t *dst;
    if (z == 0) {
        const uint8_t *src = l == 1 ? C.img0 : C.U + S.off; const int pitch = l == 1 ? C.pitch0 : S.w;
        p00 = src[(size_t)ye.x*pitch + sx]; p01 = src[(size_t)ye.x*pitch + sx1]; p10 = src[(size_t)ye.y*pitch + sx]; p11 = src[(size_t)ye.y*pitch + sx1];
        dst = C.U + G.off;
    } else {
        const int d = z - 1;
        p00 = cvo_m(C, d, l - 1, RS, sx, ye.x); p01 = cvo_m(C, d, l - 1, RS, sx1, ye.x); p10 = cvo_m(C, d, l - 1, RS, sx, ye.y); p11 = cvo_m(C, d, l - 1, RS, sx1, ye.y);
        dst = C.M + (size_t)d*C.m_stride + G.off;
    }
    const int S0 = p00*a0 + p01*a1, S1 = p10*a0 + p11*a1;
    dst[(size_t)y*G.w + x] = (uint8_t)((((ye.z*(S0 >> 4)) >> 16) + ((ye.w*(S1 >> 4)) >> 16) + 2) >> 2);
}

// GaussianBlur 7 x 7 sigma 2 of the unmasked levels, the 8-bit path of V9, REFLECT_101 at the level's edge.  One 32 x 32 tile per workgroup.
__global__ __launch_bounds__(256) void k_cvo_blur(CvoDev C) {
    __shared__ uint8_t px[38*40];
    __shared__ unsigned short hs[38*32];
    int l, tx, ty; cvo_tile(C, blockIdx.x, l, tx, ty);
    const CvoLevel &G = C.L[l];
    const uint8_t *src = l == 0 ? C.img0 : C.U + G.off; const int pitch = l == 0 ? C.pitch0 : G.w;
    const int X0 = tx*CVO_TS, Y0 = ty*CVO_TS, tid = threadIdx.x;
    for (int i = tid; i < 38*38; i += 256) { const int yy = i/38, xx = i - yy*38;
        const int gx = min(max(reflect101(X0 + xx - 3, G.w), 0), G.w - 1), gy = min(max(reflect101(Y0 + yy - 3, G.h), 0), G.h - 1);      // (the clamp: columns and rows past the level in its last tiles, never used)
        px[yy*40 + xx] = src[(size_t)gy*pitch + gx]; }
    __syncthreads();
    for (int i = tid; i < 38*32; i += 256) { const int yy = i >> 5, xx = i & 31; int s = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) s += C.gk[k]*px[yy*40 + xx + k];
        hs[i] = (unsigned short)s; }                                             // (<= 256 x 255)
    __syncthreads();
    for (int i = tid; i < 32*32; i += 256) { const int yy = i >> 5, xx = i & 31, x = X0 + xx, y = Y0 + yy; int s = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) s += C.gk[k]*hs[(yy + k)*32 + xx];
        if (x < G.w && y < G.h) C.B[G.boff + (size_t)y*G.w + x] = (uint8_t)min(max((s + (1 << 15)) >> 16, 0), 255); }
}

// cv::FAST(20, nms) of a whole masked level + runByImageBorder(31): the tile's pixels with a 4-px apron -> LDS, cornerScore of the tile and a 1-px
// ring, strict maximum over the 8 neighbours.  grid (tiles of all levels, nd).  A tile away from the footprint (dilated by FAST's radius) is empty.
__global__ __launch_bounds__(256) void k_cvo_fast(CvoDev C) {
    __shared__ __attribute__((aligned(4))) uint8_t px[40*40];
    __shared__ uint8_t sc[34*34];
    __shared__ int s_n;
    int l, tx, ty; cvo_tile(C, blockIdx.x, l, tx, ty);
    const CvoLevel &G = C.L[l];
    const int d = blockIdx.y, tid = threadIdx.x, X0 = tx*CVO_TS, Y0 = ty*CVO_TS;
    const int4 R = cvo_foot(C, d, l);
    int *cnt = C.tcnt + (size_t)d*C.ntiles + blockIdx.x;
    const int bx0 = max(X0, CVO_BORDER), bx1 = min(X0 + CVO_TS, G.w - CVO_BORDER), by0 = max(Y0, CVO_BORDER), by1 = min(Y0 + CVO_TS, G.h - CVO_BORDER);    // kept pixels [bx0, bx1) x [by0, by1)
    if (R.x > R.z || bx0 >= bx1 || by0 >= by1 || bx0 > R.z + 3 || bx1 - 1 < R.x - 3 || by0 > R.w + 3 || by1 - 1 < R.y - 3) { if (tid == 0) *cnt = 0; return; }
    for (int i = tid; i < 40*40; i += 256) { const int yy = i/40, xx = i - yy*40; px[i] = (uint8_t)cvo_m(C, d, l, R, X0 + xx - 4, Y0 + yy - 4); }
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < 34*34; i += 256) { const int yy = i/34, xx = i - yy*34, x = X0 + xx - 1, y = Y0 + yy - 1;
        int s = 0;                                                               // (FAST skips the level's first and last three rows and columns)
        if (x >= 3 && x < G.w - 3 && y >= 3 && y < G.h - 3) { const uint8_t *p = px + (yy + 3)*40 + xx + 3; if (fast_maybe(p, 40, 20)) s = fast_score(p, 40, 20); }
        sc[i] = (uint8_t)s; }
    __syncthreads();
    uint32_t *out = C.tkp + ((size_t)d*C.ntiles + blockIdx.x)*CVO_TCAP;
    for (int i = tid; i < 32*32; i += 256) { const int yy = i >> 5, xx = i & 31, x = X0 + xx, y = Y0 + yy;
        const uint8_t *q = sc + (yy + 1)*34 + xx + 1; const int s = q[0];
        if (s > 0 && x >= bx0 && x < bx1 && y >= by0 && y < by1 && s > q[-35] && s > q[-34] && s > q[-33] && s > q[-1] && s > q[1] && s > q[33] && s > q[34] && s > q[35]) {
            const int k = atomicAdd(&s_n, 1); if (k < CVO_TCAP) out[k] = (uint32_t)x | ((uint32_t)y << 10) | ((uint32_t)s << 20); } }
    __syncthreads();
    if (tid == 0) *cnt = min(s_n, CVO_TCAP);
}

// HarrisResponses (blockSize 7, k 0.04) at (x, y) of a masked level: exact int32 sums, then the one fp32 expression in the written order
__device__ float cvo_harris(const CvoDev &C, int d, int l, const int4 R, int x, int y) {
    int a = 0, b = 0, c = 0;
    int r0[9], r1[9], r2[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { r0[i] = cvo_m(C, d, l, R, x - 4 + i, y - 4); r1[i] = cvo_m(C, d, l, R, x - 4 + i, y - 3); }
    for (int j = 0; j < 7; j++) {
#pragma unroll
        for (int i = 0; i < 9; i++) r2[i] = cvo_m(C, d, l, R, x - 4 + i, y - 2 + j);
#pragma unroll
        for (int i = 0; i < 7; i++) {
            const int Ix = (r1[i+2] - r1[i])*2 + (r0[i+2] - r0[i]) + (r2[i+2] - r2[i]);
            const int Iy = (r2[i+1] - r0[i+1])*2 + (r2[i] - r0[i]) + (r2[i+2] - r0[i+2]);
            a += Ix*Ix; b += Iy*Iy; c += Ix*Iy;
        }
#pragma unroll
        for (int i = 0; i < 9; i++) { r0[i] = r1[i]; r1[i] = r2[i]; }
    }
    const float sc = __fdiv_rn(1.f, __fmul_rn(28.f, 255.f)), sc4 = __fmul_rn(__fmul_rn(__fmul_rn(sc, sc), sc), sc);
    const float fa = (float)a, fb = (float)b, fc = (float)c, s = __fadd_rn(fa, fb);
    return __fmul_rn(__fsub_rn(__fsub_rn(__fmul_rn(fa, fb), __fmul_rn(fc, fc)), __fmul_rn(__fmul_rn(0.04f, s), s)), sc4);
}

// The two retainBest cuts of one (detection, level).  grid (CVO_NL, nd).  Nothing here is bounded by a list: the corners stay in their tiles' lists,
// a cut is a threshold (every point at or above the n-th largest value stays: all ties), the survivors are counted per level row.
__global__ __launch_bounds__(256) void k_cvo_select(CvoDev C) {
    __shared__ int hist[256], rows[CVO_MAX_H], s_cnt[CVO_MAX_T];          // (s_cnt: the level's list lengths, read once: most tiles of a level are empty)
    __shared__ uint32_t s_pre; __shared__ int s_need, s_tot, s_t1;
    const int l = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CvoLevel &G = C.L[l];
    const int nt = G.ntx*G.nty, q = G.quota;
    const int *tcnt = C.tcnt + (size_t)d*C.ntiles + G.tile0;
    const uint32_t *tkp = C.tkp + ((size_t)d*C.ntiles + G.tile0)*CVO_TCAP;
    uint32_t *tkey = C.tkey + ((size_t)d*C.ntiles + G.tile0)*CVO_TCAP;
    const int4 R = cvo_foot(C, d, l);
    // ---- first cut: 2 q on the FAST score
    hist[tid] = 0;
    for (int y = tid; y < CVO_MAX_H; y += 256) rows[y] = 0;
    if (tid == 0) s_tot = 0;
    for (int t = tid; t < nt; t += 256) s_cnt[t] = min(max(tcnt[t], 0), CVO_TCAP);
    __syncthreads();
    for (int t = wv; t < nt; t += 4) { const int n = s_cnt[t]; for (int e = lane; e < n; e += 64) atomicAdd(&hist[tkp[(size_t)t*CVO_TCAP + e] >> 20], 1); }
    __syncthreads();
    if (tid == 0) { int N = 0; for (int b = 0; b < 256; b++) N += hist[b];
        int t1 = 0;
        if (q <= 0) t1 = 256;                                                    // retainBest(0): nothing stays
        else if (N > 2*q) { int acc = 0; for (int b = 255; b >= 0; b--) { acc += hist[b]; if (acc >= 2*q) { t1 = b; break; } } }
        s_t1 = t1; }
    __syncthreads();
    const int t1 = s_t1;
    // ---- Harris responses of its survivors
    for (int t = wv; t < nt; t += 4) { const int n = s_cnt[t];
        for (int e = lane; e < n; e += 64) { const uint32_t p = tkp[(size_t)t*CVO_TCAP + e];
            if ((int)(p >> 20) >= t1) { tkey[(size_t)t*CVO_TCAP + e] = cvo_key(cvo_harris(C, d, l, R, p & 1023u, (p >> 10) & 1023u)); atomicAdd(&s_tot, 1); } } }
    __syncthreads();
    // ---- second cut: q on the response = the q-th largest key, a byte at a time from the top
    uint32_t k2 = 0;
    if (s_tot > q && q > 0) {
        if (tid == 0) { s_pre = 0; s_need = q; }
        for (int r = 3; r >= 0; r--) {
            hist[tid] = 0;
            __syncthreads();
            const uint32_t pre = s_pre, hi = r == 3 ? 0u : 0xffffffffu << (8*(r + 1));
            for (int t = wv; t < nt; t += 4) { const int n = s_cnt[t];
                for (int e = lane; e < n; e += 64) { if ((int)(tkp[(size_t)t*CVO_TCAP + e] >> 20) < t1) continue;
                    const uint32_t k = tkey[(size_t)t*CVO_TCAP + e]; if ((k & hi) == pre) atomicAdd(&hist[(k >> (8*r)) & 255u], 1); } }
            __syncthreads();
            if (tid == 0) { int acc = 0, need = s_need, b = 255; for (; b > 0; b--) { if (acc + hist[b] >= need) break; acc += hist[b]; }
                s_need = need - acc; s_pre = pre | ((uint32_t)b << (8*r)); }
            __syncthreads();
        }
        k2 = s_pre;
    }
    // ---- the survivors per row, their exclusive scan
    for (int t = wv; t < nt; t += 4) { const int n = s_cnt[t];
        for (int e = lane; e < n; e += 64) { const uint32_t p = tkp[(size_t)t*CVO_TCAP + e];
            if ((int)(p >> 20) >= t1 && tkey[(size_t)t*CVO_TCAP + e] >= k2) atomicAdd(&rows[min((int)((p >> 10) & 1023u), CVO_MAX_H - 1)], 1); } }
    __syncthreads();
    if (tid == 0) { int run = 0; int *ro = C.rowoff + ((size_t)d*CVO_NL + l)*CVO_MAX_H;
        for (int y = 0; y < CVO_MAX_H; y++) { ro[y] = run; run += rows[y]; }
        C.lvlcnt[d*CVO_NL + l] = run; C.thr[2*(d*CVO_NL + l)] = (uint32_t)t1; C.thr[2*(d*CVO_NL + l) + 1] = k2; }
}

// grid (tiles of all levels, nd): a thread per entry of the tile's list.  Output order by construction: level-major, inside a level by row, then column.
__global__ __launch_bounds__(CVO_TCAP) void k_cvo_place(CvoDev C) {
    int l, tx, ty; cvo_tile(C, blockIdx.x, l, tx, ty);
    const CvoLevel &G = C.L[l];
    const int d = blockIdx.y, e = threadIdx.x;
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < CVO_NL; k++) { const int n = C.lvlcnt[d*CVO_NL + k]; before += k < l ? n : 0; total += n; }
    if (blockIdx.x == 0 && e == 0) C.o_cnt[d] = total;
    if (total > C.cap) return;                                                   // (the host reports it; nothing is written for this detection)
    const int *tcnt = C.tcnt + (size_t)d*C.ntiles + G.tile0;
    const uint32_t *tkp = C.tkp + ((size_t)d*C.ntiles + G.tile0)*CVO_TCAP, *tkey = C.tkey + ((size_t)d*C.ntiles + G.tile0)*CVO_TCAP;
    const int t = ty*G.ntx + tx;
    if (e >= min(tcnt[t], CVO_TCAP)) return;
    const uint32_t t1 = C.thr[2*(d*CVO_NL + l)], k2 = C.thr[2*(d*CVO_NL + l) + 1];
    const uint32_t p = tkp[(size_t)t*CVO_TCAP + e], key = tkey[(size_t)t*CVO_TCAP + e];
    if ((p >> 20) < t1 || key < k2) return;
    const uint32_t x = p & 1023u, y = (p >> 10) & 1023u;
    int left = 0;
    for (int u = 0; u < G.ntx; u++) { const int t2 = ty*G.ntx + u, n = min(tcnt[t2], CVO_TCAP);
        for (int j = 0; j < n; j++) { const uint32_t p2 = tkp[(size_t)t2*CVO_TCAP + j];
            if (((p2 >> 10) & 1023u) == y && (p2 & 1023u) < x && (p2 >> 20) >= t1 && tkey[(size_t)t2*CVO_TCAP + j] >= k2) left++; } }
    const int o = before + C.rowoff[((size_t)d*CVO_NL + l)*CVO_MAX_H + min((int)y, CVO_MAX_H - 1)] + left;
    if (o < C.cap) C.sel[(size_t)d*C.cap + o] = make_float4((float)x, (float)y, cvo_unkey(key), (float)l);
}

// grid (CVO_DESC_BLOCKS, nd), eight keypoints per workgroup pass, 32 lanes each: lanes 0 .. 15 the rows +-v of IC_Angle's patch on the MASKED level (detect),
// lane i byte i of the descriptor on the blurred UNMASKED level (compute).  Results go straight into the arrays the host hands out (cvo_launch's output pointers).
__global__ __launch_bounds__(256) void k_cvo_describe(CvoDev C) {
    const int d = blockIdx.y, lane = threadIdx.x & 31, sub = threadIdx.x >> 5;
    int total = 0;
#pragma unroll
    for (int k = 0; k < CVO_NL; k++) total += C.lvlcnt[d*CVO_NL + k];
    if (total > C.cap) return;
    for (int o = blockIdx.x*8 + sub; o < total; o += 8*CVO_DESC_BLOCKS) {        // (total <= cap)
        const float4 sv = C.sel[(size_t)d*C.cap + o];
        const int l = min(max((int)sv.w, 0), CVO_NL - 1), x = (int)sv.x, y = (int)sv.y;
        const CvoLevel &G = C.L[l];
        const int4 R = cvo_foot(C, d, l);
        int m10 = 0, m01 = 0;
        if (lane < 16) { const int v = lane, dd = v == 0 ? 15 : C.umax[v]; int vs = 0;
            for (int u = -dd; u <= dd; u++) { const int vp = cvo_m(C, d, l, R, x + u, y + v), vm = cvo_m(C, d, l, R, x + u, y - v); vs += vp - vm; m10 += u*(v == 0 ? vp : vp + vm); }
            m01 = v*vs; }
#pragma unroll
        for (int w = 8; w > 0; w >>= 1) { m10 += __shfl_xor(m10, w, 16); m01 += __shfl_xor(m01, w, 16); }
        m10 = __shfl(m10, 0, 32); m01 = __shfl(m01, 0, 32);
        const float angle = fast_atan2f_dev((float)m01, (float)m10);
        const float ptx = __fmul_rn((float)x, G.scale), pty = __fmul_rn((float)y, G.scale);
        float a = 0.f, b = 0.f;
        if (lane == 0) { const float rad = __fmul_rn(angle, (float)(3.14159265358979323846/180.f)); a = (float)cos((double)rad); b = (float)sin((double)rad); }
        a = __shfl(a, 0, 32); b = __shfl(b, 0, 32);
        const int cx = (int)rintf(__fmul_rn(ptx, G.inv)), cy = (int)rintf(__fmul_rn(pty, G.inv));
        const uint8_t *bl = C.B + G.boff;
        const int8_t *pat = d_pattern + 32*lane;
        int val = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const float x0 = pat[4*t], y0 = pat[4*t+1], x1 = pat[4*t+2], y1 = pat[4*t+3];
            const int ax = cx + (int)rintf(__fsub_rn(__fmul_rn(x0, a), __fmul_rn(y0, b))), ay = cy + (int)rintf(__fadd_rn(__fmul_rn(x0, b), __fmul_rn(y0, a)));
            const int bx = cx + (int)rintf(__fsub_rn(__fmul_rn(x1, a), __fmul_rn(y1, b))), by = cy + (int)rintf(__fadd_rn(__fmul_rn(x1, b), __fmul_rn(y1, a)));
            const int t0 = bl[(size_t)min(max(ay, 0), G.h - 1)*G.w + min(max(ax, 0), G.w - 1)], t1 = bl[(size_t)min(max(by, 0), G.h - 1)*G.w + min(max(bx, 0), G.w - 1)];     // (a keypoint is 31 px inside its level, a tap at most 19 from it: the clamp never acts)
            val |= (t0 < t1) << t;
        }
        C.o_desc[((size_t)d*C.cap + o)*32 + lane] = (uint8_t)val;
        if (lane < 6) C.o_kp[((size_t)d*C.cap + o)*6 + lane] = lane == 0 ? ptx : lane == 1 ? pty : lane == 2 ? __fmul_rn(31.f, G.scale) : lane == 3 ? angle : lane == 4 ? sv.z : (float)l;
    }
}
