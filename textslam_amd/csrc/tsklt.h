// tsklt.h -- tracking::TrackNewTextFeat -> cv::calcOpticalFlowPyrLK on the resident pyramids of two contexts: one launch for all points and
// all levels (include/tsframe.h: tsframe_klt_track; the arithmetic is docs/klt_recalled.md, restated on the CPU by tests/klt_ref.py).
// A wave per point, four points per workgroup, no LDS and no barrier: a point's result cannot depend on its neighbours.  Lane t owns the
// window pixels t, t + 64, ... (row-major); Iw, Ix, Iy of the level stay in its registers over the iterations; each iteration gathers the four
// bilinear taps of J per pixel (L2 hits).  The five window sums are exact integers: int32 per lane (at most 16 terms below 2^25), int64
// across the wave by a butterfly, so every lane holds the same sum whatever the order; one rounding to fp32.  The 2x2 solve and every exit
// decision are then computed by all lanes on identical values (made uniform for the compiler by readfirstlane): the branches are wave-uniform,
// a point that fails a test only skips work.  Every loop has a static bound: levels <= 8, iterations <= 100, NPER pixels per lane, four
// reflection folds (enough because a level is larger than the window, see klt_reflect).
#ifndef TSKLT_H
#define TSKLT_H

#define KLT_WAVES 4
struct KltArgs {
    const uint8_t *I[TSFRAME_MAX_LEVELS], *J[TSFRAME_MAX_LEVELS];
    int w[TSFRAME_MAX_LEVELS], h[TSFRAME_MAX_LEVELS];
    int n, n_levels, win, max_iter;
    float eps2, min_eig;
};

// BORDER_REFLECT_101 for -n <= p <= 2n - 1 with n >= 4 (what a window that passed the range test on a level larger than the window can ask
// for): three folds at most.  The clamp only guarantees an in-bounds read should a caller ever break that precondition.
__device__ __forceinline__ int klt_reflect(int p, int n) {
#pragma unroll
    for (int k = 0; k < 4; k++) { if (p < 0) p = -p; else if (p >= n) p = 2*n - 2 - p; }
    return min(max(p, 0), n - 1);
}

// the range test, in fp32 before any integer conversion: floor(p) in [-win, cols) x [-win, rows), finite, |coordinate| < 2^20
__device__ __forceinline__ bool klt_in_range(float x, float y, int win, int w, int h, int &ix, int &iy) {
    const float fx = floorf(x), fy = floorf(y);
    const bool ok = fabsf(x) < 1048576.0f && fabsf(y) < 1048576.0f && fx >= (float)(-win) && fx < (float)w && fy >= (float)(-win) && fy < (float)h;
    ix = ok ? (int)fx : 0; iy = ok ? (int)fy : 0;
    return ok;
}

__device__ __forceinline__ void klt_weights(float a, float b, int &w00, int &w01, int &w10, int &w11) {
    const float s = 16384.0f;
    w00 = (int)rintf((1.0f - a)*(1.0f - b)*s); w01 = (int)rintf(a*(1.0f - b)*s); w10 = (int)rintf((1.0f - a)*b*s);
    w11 = 16384 - w00 - w01 - w10;
}

__device__ __forceinline__ float klt_wave_sum(int v) {                 // exact int64 sum over the wave, rounded once to fp32
    long long s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const int lo = __builtin_amdgcn_readfirstlane((int)(unsigned)(s & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(s >> 32));
    return (float)(long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// the bilinear blend of the image at the window pixel (x, y): intensity x 32
template <bool REFLECT>
__device__ __forceinline__ int klt_blend_img(const uint8_t *__restrict__ img, int w, int h, int x, int y, int w00, int w01, int w10, int w11) {
    const int x0 = REFLECT ? klt_reflect(x, w) : x, x1 = REFLECT ? klt_reflect(x + 1, w) : x + 1;
    const int y0 = REFLECT ? klt_reflect(y, h) : y, y1 = REFLECT ? klt_reflect(y + 1, h) : y + 1;
    const uint8_t *r0 = img + (size_t)y0*w, *r1 = img + (size_t)y1*w;
    return ((int)r0[x0]*w00 + (int)r0[x1]*w01 + (int)r1[x0]*w10 + (int)r1[x1]*w11 + 256) >> 9;
}

// Iw, Ix, Iy of the window pixel (x, y) of I: the 4 x 4 patch around it gives the Scharr derivatives at its four bilinear taps (the image
// continues by REFLECT_101, the derivative is 0 outside the image)
template <bool REFLECT>
__device__ __forceinline__ void klt_blend_ref(const uint8_t *__restrict__ img, int w, int h, int x, int y, int w00, int w01, int w10, int w11,
                                              int &Iw, int &Ix, int &Iy) {
    int P[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint8_t *row = img + (size_t)(REFLECT ? klt_reflect(y - 1 + r, h) : y - 1 + r)*w;
#pragma unroll
        for (int c = 0; c < 4; c++) P[r][c] = row[REFLECT ? klt_reflect(x - 1 + c, w) : x - 1 + c];
    }
    int dx[2][2], dy[2][2];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const bool in = !REFLECT || ((unsigned)(x + c) < (unsigned)w && (unsigned)(y + r) < (unsigned)h);
            const int sl = 3*P[r][c] + 10*P[r + 1][c] + 3*P[r + 2][c], sr = 3*P[r][c + 2] + 10*P[r + 1][c + 2] + 3*P[r + 2][c + 2];
            const int tu = 3*P[r][c] + 10*P[r][c + 1] + 3*P[r][c + 2], td = 3*P[r + 2][c] + 10*P[r + 2][c + 1] + 3*P[r + 2][c + 2];
            dx[r][c] = in ? sr - sl : 0; dy[r][c] = in ? td - tu : 0;
        }
    Iw = (P[1][1]*w00 + P[1][2]*w01 + P[2][1]*w10 + P[2][2]*w11 + 256) >> 9;
    Ix = (dx[0][0]*w00 + dx[0][1]*w01 + dx[1][0]*w10 + dx[1][1]*w11 + 8192) >> 14;
    Iy = (dy[0][0]*w00 + dy[0][1]*w01 + dy[1][0]*w10 + dy[1][1]*w11 + 8192) >> 14;
}

template <int NPER>                                                    // window pixels per lane: win * win <= 64 * NPER
__global__ __launch_bounds__(64*KLT_WAVES) void k_klt_track(KltArgs A, const float *__restrict__ prev_xy, float *__restrict__ next_xy, uint8_t *__restrict__ status) {
    const int lane = threadIdx.x & 63, pt = blockIdx.x*KLT_WAVES + (threadIdx.x >> 6);
    if (pt >= A.n) return;                                             // (the whole wave)
    const float ptx = prev_xy[2*pt], pty = prev_xy[2*pt + 1];
    if (!(fabsf(ptx) < INFINITY) || !(fabsf(pty) < INFINITY)) {        // a non-finite input point: status 0, the input handed back
        if (lane == 0) { next_xy[2*pt] = ptx; next_xy[2*pt + 1] = pty; status[pt] = 0; }
        return;
    }
    const int win = A.win, ww = win*win;
    const float half = (float)((win - 1)/2);
    int wx[NPER], wy[NPER]; bool live[NPER];
#pragma unroll
    for (int k = 0; k < NPER; k++) {
        const int idx = lane + 64*k;
        live[k] = idx < ww;
        wy[k] = live[k] ? idx/win : 0; wx[k] = live[k] ? idx - wy[k]*win : 0;      // a slot past the window aliases pixel (0, 0) with Ix = Iy = 0
    }
    float nx = 0.0f, ny = 0.0f, ox = 0.0f, oy = 0.0f;
    int st = 1;
    for (int l = A.n_levels - 1; l >= 0; l--) {
        const uint8_t *__restrict__ I = A.I[l], *__restrict__ J = A.J[l];
        const int w = A.w[l], h = A.h[l];
        const float sc = __int_as_float((127 - l) << 23);              // 2^-l
        float px = ptx*sc, py = pty*sc;
        if (l == A.n_levels - 1) { nx = px; ny = py; } else { nx = nx*2.0f; ny = ny*2.0f; }
        ox = nx; oy = ny;
        px = px - half; py = py - half;
        int ix, iy;
        if (!klt_in_range(px, py, win, w, h, ix, iy)) { if (l == 0) st = 0; continue; }
        int w00, w01, w10, w11;
        klt_weights(px - (float)ix, py - (float)iy, w00, w01, w10, w11);
        int Iw[NPER], Ix[NPER], Iy[NPER];
        int s11 = 0, s12 = 0, s22 = 0;
        const bool inner = ix >= 1 && iy >= 1 && ix + win + 1 < w && iy + win + 1 < h;   // the window and its Scharr ring inside the image
#pragma unroll
        for (int k = 0; k < NPER; k++) {
            if (inner) klt_blend_ref<false>(I, w, h, ix + wx[k], iy + wy[k], w00, w01, w10, w11, Iw[k], Ix[k], Iy[k]);
            else klt_blend_ref<true>(I, w, h, ix + wx[k], iy + wy[k], w00, w01, w10, w11, Iw[k], Ix[k], Iy[k]);
            if (!live[k]) { Iw[k] = 0; Ix[k] = 0; Iy[k] = 0; }
            s11 += Ix[k]*Ix[k]; s12 += Ix[k]*Iy[k]; s22 += Iy[k]*Iy[k];
        }
        const float scale = 1.0f/1048576.0f;                            // 2^-20
        const float A11 = klt_wave_sum(s11)*scale, A12 = klt_wave_sum(s12)*scale, A22 = klt_wave_sum(s22)*scale;
        float D = A11*A22 - A12*A12;
        const float dd = A11 - A22;
        const float min_eig = ((A22 + A11) - sqrtf(dd*dd + (4.0f*A12)*A12))/(float)(2*win*win);
        if (min_eig < A.min_eig || D < 1.1920928955078125e-7f) { if (l == 0) st = 0; continue; }
        D = 1.0f/D;
        nx = nx - half; ny = ny - half;
        float pdx = 0.0f, pdy = 0.0f;
        for (int j = 0; j < A.max_iter; j++) {
            int jx, jy;
            if (!klt_in_range(nx, ny, win, w, h, jx, jy)) { if (l == 0) st = 0; break; }
            klt_weights(nx - (float)jx, ny - (float)jy, w00, w01, w10, w11);
            const bool jin = jx >= 0 && jy >= 0 && jx + win < w && jy + win < h;
            int sb1 = 0, sb2 = 0;
#pragma unroll
            for (int k = 0; k < NPER; k++) {
                const int Jw = jin ? klt_blend_img<false>(J, w, h, jx + wx[k], jy + wy[k], w00, w01, w10, w11)
                                   : klt_blend_img<true>(J, w, h, jx + wx[k], jy + wy[k], w00, w01, w10, w11);
                const int diff = Jw - Iw[k];
                sb1 += diff*Ix[k]; sb2 += diff*Iy[k];
            }
            const float b1 = klt_wave_sum(sb1)*scale, b2 = klt_wave_sum(sb2)*scale;
            const float dx = (A12*b2 - A22*b1)*D, dy = (A12*b1 - A11*b2)*D;
            nx = nx + dx; ny = ny + dy;
            ox = nx + half; oy = ny + half;
            if (dx*dx + dy*dy <= A.eps2) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) { ox = ox - dx*0.5f; oy = oy - dy*0.5f; break; }
            pdx = dx; pdy = dy;
        }
        nx = ox; ny = oy;
    }
    if (st) { int jx, jy; if (!klt_in_range(ox - half, oy - half, win, A.w[0], A.h[0], jx, jy)) st = 0; }
    if (lane == 0) { next_xy[2*pt] = ox; next_xy[2*pt + 1] = oy; status[pt] = (uint8_t)st; }
}
#endif
