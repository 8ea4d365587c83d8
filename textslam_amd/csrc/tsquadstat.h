// tsquadstat.h -- tool::CalTextinfo (src/tool.cc:1178-1262) on the device, stated once for the BA library (mu / sigma of a projected text box: musigma_core,
// tsba_kernels_lin.h) and the frame front-end (k_object_info, tsobj.h): the integer histogram of the pixels of a clamped box that the filled quad covers, then
// n, mu and sigma from its 256 bins; with it the fixed-order workgroup reductions both libraries sum with.  Device code only (included after tsraster.h).
#pragma once
__device__ __forceinline__ double wave_sum1(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int NT>
__device__ __forceinline__ double block_sum(double v, double *lds) {     // deterministic (fixed order), NT threads, all get the result
    const int t = threadIdx.x;
    lds[t] = v; __syncthreads();
    if (t < 64) {
        double s = lds[t];
#pragma unroll
        for (int k = 64; k < NT; k += 64) s += lds[t + k];
        s = wave_sum1(s);
        if (t == 0) lds[0] = s;
    }
    __syncthreads();
    const double r = lds[0]; __syncthreads();
    return r;
}
template <int NT>
__device__ __forceinline__ double block_max(double v, double *lds) {
    const int t = threadIdx.x;
    lds[t] = v; __syncthreads();
    if (t < 64) {
        double s = lds[t];
#pragma unroll
        for (int k = 64; k < NT; k += 64) s = fmax(s, lds[t + k]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = fmax(s, __shfl_xor(s, o, 64));
        if (t == 0) lds[0] = s;
    }
    __syncthreads();
    const double r = lds[0]; __syncthreads();
    return r;
}

#ifdef MID_STAMPS                           // (tools/mid_stamps.sh: cycles of a mu / sigma workgroup by phase into W.dbg[56..63] -- the slots of k_schur_t's gradient rows in that build)
#define MS_STAMP(slot) do { if (threadIdx.x == 0 && dbg) atomicAdd((unsigned long long *)&dbg[56 + (slot)], (unsigned long long)(clock64() - us_t0)); } while (0)
#else
#define MS_STAMP(slot) do { } while (0)
#endif

// n, mu and sigma of the pixels of the box [xMin, xMax] x [yMin, yMax] (clamped to the w x hh image img, uniform in the workgroup) that cv::fillPoly of the quad
// s_xy (eight integer corners in LDS) covers; the three values in every one of the NT >= 256 threads, n < 2 (or an empty box) as mu = sigma = 0.
// The mask is built and read in bands of B = MS_MASK_WORDS*32 / w rows that start at yMin (raster_quad_rows: a window of the FULL image's rows), so a box no
// taller than B rows -- any box of a level of at most 640 x 480 -- costs one band, and only the band's words are cleared.  The moments come from the integer
// histogram: the same bits whatever the order of the pixels and however they are banded; the bins are summed through block_sum<NT> (the slots past 255 add
// +0.0, so every NT gives the bits of NT = 256).  n and the sum are exact integers, so mu is exact.
// A box of one band leaves that band's mask in LDS on return: pixel (x, y) at bit (y - yMin) w + x (k_object_info's pixel stage reads it).
// LDS: mask [MS_MASK_WORDS], hist [256], s_red [NT].  The caller synchronises between writing s_xy and the call.
struct QuadMoments { double n, mu, sigma; };
template <int NT>
__device__ __forceinline__ QuadMoments quad_moments(const uint8_t *__restrict__ img, int w, int hh, const int *s_xy, int xMin, int xMax, int yMin, int yMax,
                                                    unsigned *mask, unsigned *hist, double *s_red
#ifdef MID_STAMPS
                                                    , long long *dbg, long long us_t0       // (stamps 2 - 4 and the fill's own are taken at the first band)
#endif
                                                    ) {
    const int tid = threadIdx.x;
    if (tid < 256) hist[tid] = 0;
    const int bw = xMax - xMin + 1, B = (MS_MASK_WORDS*32)/w;
    if (bw > 0)
        for (int yb = yMin; yb <= yMax; yb += B) {
            const int ye = min(yb + B, yMax + 1), bh = ye - yb;
            for (int k = tid; k < (bh*w + 31) >> 5; k += NT) mask[k] = 0;
            __syncthreads();
#ifdef MID_STAMPS
            if (yb == yMin) MS_STAMP(2);                          // (mask cleared)
            raster_quad_rows(mask, s_xy, w, hh, yb, ye, tid, NT, dbg && yb == yMin ? dbg + 48 : nullptr);
#else
            raster_quad_rows(mask, s_xy, w, hh, yb, ye, tid, NT);
#endif
            __syncthreads();
#ifdef MID_STAMPS
            if (yb == yMin) MS_STAMP(3);                          // (quad rasterised)
#endif
            // histogram of the band's masked pixels inside the box (tool.cc:1217-1232): four pixels per thread and round with their loads in flight
            // together; (x, y) advance without a division per pixel
            const uint8_t *__restrict__ band = img + (size_t)yb*w;
            const int npx = bw*bh, dx = NT % bw, dy = NT / bw;
            int x = tid % bw, y = tid / bw;
            for (int k0 = tid; k0 < npx; k0 += 4*NT) {
                int bit[4]; bool in[4]; unsigned px[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    bit[u] = y*w + xMin + x;                      // (band-relative, in the mask and in the image)
                    in[u] = k0 + u*NT < npx && (mask[bit[u] >> 5] & (1u << (bit[u] & 31)));
                    x += dx; y += dy; if (x >= bw) { x -= bw; y++; }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) px[u] = in[u] ? band[bit[u]] : 0u;
#pragma unroll
                for (int u = 0; u < 4; u++) if (in[u]) atomicAdd(&hist[px[u]], 1u);
            }
            __syncthreads();
#ifdef MID_STAMPS
            if (yb == yMin) MS_STAMP(4);                          // (histogram)
#endif
        }
    const double hv = tid < 256 ? (double)hist[tid] : 0.0;
    QuadMoments M = { 0.0, 0.0, 0.0 };
    M.n = block_sum<NT>(hv, s_red);
    const double sm = block_sum<NT>(hv*(double)tid, s_red);
    if (M.n < 2.0) return M;
    M.mu = sm/M.n;
    const double d = (double)tid - M.mu;
    M.sigma = sqrt(block_sum<NT>(hv*d*d, s_red)/(M.n - 1.0));
    return M;
}
