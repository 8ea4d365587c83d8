// tsundist.h -- the camera-frame entry of libtsframe.so (included by tsframe.hip): cv::undistort's fixed-point map, built once per camera, and the
// per-frame remap + grey conversion that leaves level 0 of the BA pyramid in place.  The arithmetic is docs/undistort_recalled.md (U1 - U7), the CPU
// restatement tests/camera_frame_ref.py; the fp64 part is compiled without FMA contraction like the rest of the library, everything after it is integer.
#ifndef TSUNDIST_H
#define TSUNDIST_H

struct UndistCam { double K[4], dist[5], Kn[4]; int w, h, s0; };      // K, K_new = fx fy cx cy; dist = k1 k2 p1 p2 k3; s0 = rows per strip (U1)

// U5: saturate_cast<int>(double): round half to even, clamped to int; NaN gives INT_MIN
__device__ __forceinline__ int undist_saturate_int(double t) {
    if (t != t) return INT_MIN;
    const double r = rint(t);
    return r >= 2147483647.0 ? INT_MAX : r <= -2147483648.0 ? INT_MIN : (int)r;
}

// U1 - U5 literally: one thread per image row runs that row's serial chain (once per camera: its cost does not matter).  Every loop is bounded by w.
__global__ __launch_bounds__(64) void k_undist_map(UndistCam C, int16_t *__restrict__ xy, uint16_t *__restrict__ frac) {
    const int row = blockIdx.x*64 + threadIdx.x;
    if (row >= C.h) return;
    const int y0 = (row/C.s0)*C.s0;
    const double i = (double)(row - y0);
    // U1: Ar of the strip; U2: cv::invert's closed form
    const double a[3][3] = { { C.Kn[0], 0.0, C.Kn[2] }, { 0.0, C.Kn[1], C.Kn[3] - (double)y0 }, { 0.0, 0.0, 1.0 } };
    const double det = a[0][0]*(a[1][1]*a[2][2] - a[1][2]*a[2][1]) - a[0][1]*(a[1][0]*a[2][2] - a[1][2]*a[2][0]) + a[0][2]*(a[1][0]*a[2][1] - a[1][1]*a[2][0]);
    const double d = 1.0/det;
    const double ir[9] = { (a[1][1]*a[2][2] - a[1][2]*a[2][1])*d, (a[0][2]*a[2][1] - a[0][1]*a[2][2])*d, (a[0][1]*a[1][2] - a[0][2]*a[1][1])*d,
                           (a[1][2]*a[2][0] - a[1][0]*a[2][2])*d, (a[0][0]*a[2][2] - a[0][2]*a[2][0])*d, (a[0][2]*a[1][0] - a[0][0]*a[1][2])*d,
                           (a[1][0]*a[2][1] - a[1][1]*a[2][0])*d, (a[0][1]*a[2][0] - a[0][0]*a[2][1])*d, (a[0][0]*a[1][1] - a[0][1]*a[1][0])*d };
    const double fx = C.K[0], fy = C.K[1], cx = C.K[2], cy = C.K[3], k1 = C.dist[0], k2 = C.dist[1], p1 = C.dist[2], p2 = C.dist[3], k3 = C.dist[4];
    double _x = i*ir[1] + ir[2], _y = i*ir[4] + ir[5], _w = i*ir[7] + ir[8];      // U3
    const size_t base = (size_t)row*C.w;
    for (int j = 0; j < C.w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        const double w_ = 1.0/_w, x = _x*w_, y = _y*w_;                           // U4
        const double x2 = x*x, y2 = y*y, r2 = x2 + y2, _2xy = 2*x*y;
        const double kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2)/(1 + ((0.0*r2 + 0.0)*r2 + 0.0)*r2);
        const double xd = x*kr + p1*_2xy + p2*(r2 + 2*x2);
        const double yd = y*kr + p1*(r2 + 2*y2) + p2*_2xy;
        const double u = fx*xd + cx, v = fy*yd + cy;
        const int iu = undist_saturate_int(u*32), iv = undist_saturate_int(v*32);  // U5
        xy[2*(base + j)] = (int16_t)(iu >> 5); xy[2*(base + j) + 1] = (int16_t)(iv >> 5);
        frac[base + j] = (uint16_t)((iv & 31)*32 + (iu & 31));
    }
}

// U6 + U7, the per-frame hot path.  A thread owns the four pixels [4t, 4t + 4) of the image taken as one row-major run, so the map entries come as
// one 16-byte and one 8-byte load and level 0 goes out as a dword whatever the width is (the map buffers are padded to a multiple of four entries).
// The output position is never needed: a pixel is its map entry.  Every tap is tested against the image before its address is formed, so nothing
// that the map could hold leads to a read outside raw's (h - 1) * stride + w * CH bytes.  CH = bytes per pixel of raw; r_first: channel 0 is red (RGB).
template <int CH, bool COLOUR>
__global__ __launch_bounds__(256) void k_undist_grey(const uint8_t *__restrict__ raw, int w, int h, int stride, int r_first,
                                                     const int16_t *__restrict__ xy, const uint16_t *__restrict__ frac, int npix,
                                                     uint8_t *__restrict__ grey, uint8_t *__restrict__ colour) {
    const int p0 = (blockIdx.x*256 + threadIdx.x)*4;
    if (p0 >= npix) return;
    const uint4 m4 = *(const uint4 *)(xy + 2*(size_t)p0);
    const uint2 f2 = *(const uint2 *)(frac + p0);
    const uint32_t m[4] = { m4.x, m4.y, m4.z, m4.w };
    const uint32_t f[4] = { f2.x & 0xffffu, f2.x >> 16, f2.y & 0xffffu, f2.y >> 16 };
    uint8_t g[4], c[4*CH];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int sx = (int16_t)(m[k] & 0xffffu), sy = (int16_t)(m[k] >> 16);
        const int a = (int)(f[k] & 31u), b = (int)((f[k] >> 5) & 31u);
        const int wt[4] = { (32 - a)*(32 - b)*32, a*(32 - b)*32, (32 - a)*b*32, a*b*32 };      // sum 32768
        const bool xin[2] = { sx >= 0 && sx < w, sx + 1 >= 0 && sx + 1 < w }, yin[2] = { sy >= 0 && sy < h, sy + 1 >= 0 && sy + 1 < h };
        int acc[CH];
#pragma unroll
        for (int ch = 0; ch < CH; ch++) acc[ch] = 16384;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (!(xin[t & 1] && yin[t >> 1])) continue;                                        // BORDER_CONSTANT 0
            const uint8_t *s = raw + (size_t)(sy + (t >> 1))*(size_t)stride + (size_t)(sx + (t & 1))*CH;
#pragma unroll
            for (int ch = 0; ch < CH; ch++) acc[ch] += wt[t]*(int)s[ch];
        }
#pragma unroll
        for (int ch = 0; ch < CH; ch++) c[k*CH + ch] = (uint8_t)(acc[ch] >> 15);
        if (CH == 1) g[k] = c[k];
        else { const int B = c[k*CH + (r_first ? 2 : 0)], G = c[k*CH + 1], R = c[k*CH + (r_first ? 0 : 2)];
               g[k] = (uint8_t)((1868*B + 9617*G + 4899*R + 8192) >> 14); }
    }
    if (p0 + 4 <= npix) {
        *(uint32_t *)(grey + p0) = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[2] << 16) | ((uint32_t)g[3] << 24);
        if (COLOUR) {
            uint32_t *o = (uint32_t *)(colour + (size_t)p0*CH);
#pragma unroll
            for (int q = 0; q < CH; q++) o[q] = (uint32_t)c[4*q] | ((uint32_t)c[4*q + 1] << 8) | ((uint32_t)c[4*q + 2] << 16) | ((uint32_t)c[4*q + 3] << 24);
        }
    } else {                                                                                   // the image's last one to three pixels
#pragma unroll
        for (int k = 0; k < 3; k++) if (p0 + k < npix) {
            grey[p0 + k] = g[k];
            if (COLOUR) {
#pragma unroll
                for (int ch = 0; ch < CH; ch++) colour[(size_t)(p0 + k)*CH + ch] = c[k*CH + ch];
            }
        }
    }
}

#endif
