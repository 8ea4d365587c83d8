// tsraster.h -- cv::fillPoly scan conversion of one quad on the device, shared by the BA library (mu / sigma of a projected text
// box, text label image: tool::CalTextinfo, tool::TextBoxWithFill) and the frame front-end (tool::GetBoxAllPixs).
// OpenCV semantics restated: boundary with cv::LineIterator (8-connected, after cv::clipLine), interior with FillEdgeCollection
// (16.16 fixed-point scanline spans).
#pragma once
#include <hip/hip_runtime.h>
__device__ int clip_line_dev(long long Wd, long long Hd, long long &x1, long long &y1, long long &x2, long long &y2) {
    long long right = Wd - 1, bottom = Hd - 1;
    int c1 = (x1 < 0) + (x1 > right)*2 + (y1 < 0)*4 + (y1 > bottom)*8;
    int c2 = (x2 < 0) + (x2 > right)*2 + (y2 < 0)*4 + (y2 > bottom)*8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) { a = c1 < 8 ? 0 : bottom; x1 += (long long)((double)(a - y1)*(double)(x2 - x1)/(double)(y2 - y1)); y1 = a; c1 = (x1 < 0) + (x1 > right)*2; }
        if (c2 & 12) { a = c2 < 8 ? 0 : bottom; x2 += (long long)((double)(a - y2)*(double)(x2 - x1)/(double)(y2 - y1)); y2 = a; c2 = (x2 < 0) + (x2 > right)*2; }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) { a = c1 == 1 ? 0 : right; y1 += (long long)((double)(a - x1)*(double)(y2 - y1)/(double)(x2 - x1)); x1 = a; c1 = 0; }
            if (c2) { a = c2 == 1 ? 0 : right; y2 += (long long)((double)(a - x2)*(double)(y2 - y1)/(double)(x2 - x1)); x2 = a; c2 = 0; }
        }
    }
    return (c1 | c2) == 0;
}
// C's truncating num / den for |num| < 2^52, 0 < |den| < 2^32 (16.16 fixed-point slopes of edges between int pixel coordinates: |num| <= 2^48) by ONE fp64 division
// and an exact correction from the remainder: the compiler's expansion of a 64-bit integer division is a long-division loop of several hundred instructions,
// and a scanline fill does four of them per thread (round 6: the quad was 30 k of a mu / sigma workgroup's 55 k cycles).  The rounded quotient of two exactly
// represented integers is within 2^-5 of the true one here, so its truncation is off by at most one; the remainder says which way.
__device__ __forceinline__ long long div_trunc_small(long long num, long long den) {
    long long q = (long long)((double)num/(double)den);
    const long long r = num - q*den, ad = den < 0 ? -den : den;
    const long long rs = num < 0 ? -r : r;                     // the remainder must carry the sign of num: rs in [0, |den|)
    const long long sq = ((num < 0) != (den < 0)) ? -1 : 1;
    if (rs < 0) q -= sq; else if (rs >= ad) q += sq;
    return q;
}
#define MS_MASK_WORDS 9600        /* 640*480/32 bits */
// The fill is stated once, as pieces; the three callers below only choose which pixels they ask about.  Integer types as OpenCV's: long long for coordinates and
// 16.16 values, int for a line's major / minor / ci.
// Boundary edge e (corner e-1 to corner e) after cv::clipLine on the FULL w x hh image (a band is never an image of its own), oriented left to right: the
// cv::LineIterator (8-connected) steps major times along its major axis from (x1, y1).
struct QuadLine { long long x1, y1, sy; int major, minor; bool steep, ok; };
__device__ __forceinline__ QuadLine quad_line(const int *xy8, int e, int w, int hh) {
    const int i0 = (e + 3) & 3;
    long long x1 = xy8[2*i0], y1 = xy8[2*i0+1], x2 = xy8[2*e], y2 = xy8[2*e+1];
    QuadLine L = { 0, 0, 1, 0, 0, false, true };
    if ((unsigned long long)x1 >= (unsigned long long)w || (unsigned long long)x2 >= (unsigned long long)w ||
        (unsigned long long)y1 >= (unsigned long long)hh || (unsigned long long)y2 >= (unsigned long long)hh)
        L.ok = clip_line_dev(w, hh, x1, y1, x2, y2);
    if (!L.ok) return L;
    long long dx = x2 - x1, dy = y2 - y1;
    if (dx < 0) { dx = -dx; dy = -dy; x1 = x2; y1 = y2; }
    L.sy = dy < 0 ? -1 : 1; if (dy < 0) dy = -dy;
    L.steep = dy > dx;
    L.major = (int)(L.steep ? dy : dx); L.minor = (int)(L.steep ? dx : dy);
    L.x1 = x1; L.y1 = y1;
    return L;
}
// Pixel i of a line, 0 <= i <= major.  The iterator's error recurrence  err += -2 minor + (err < 0 ? 2 major : 0)  has the closed form "minor steps taken before
// pixel i" = round-half-down(minor i / major) = floor((2 minor i + major - 1) / (2 major)), so the pixels of a line are independent.
__device__ __forceinline__ void quad_line_pixel(const QuadLine &L, int i, long long &x, long long &y) {
    const int ci = L.major > 0 ? (2*L.minor*i + L.major - 1)/(2*L.major) : 0;     // (clipped coordinates: < 2^21)
    x = L.steep ? L.x1 + ci : L.x1 + i; y = L.steep ? L.y1 + L.sy*i : L.y1 + L.sy*ci;
}
// Scanline interior (FillEdgeCollection).  Round 6: no array is indexed by a run-time value -- the compacted edge list and the insertion sort of a row's
// crossings put 64 bytes per lane in SCRATCH (global memory: every xs[k] of the sort a dependent round trip; the quad took 30 k of a mu / sigma workgroup's
// 55 k cycles, tools/mid_stamps.sh).  The four edges keep their slots with a validity flag, a row's (at most four) crossings are sorted by a five-exchange network
// with "no crossing" = +infinity: the same spans -- pairs of the sorted crossings, a third one ignored.
// The rows y_lo <= y < y_hi have crossings: none if fewer than two edges are valid or the quad is wholly above or below the image.
struct QuadEdges { long long ex[4], edx[4]; int ey0[4], ey1[4]; bool ev[4]; int y_lo, y_hi; };
__device__ __forceinline__ QuadEdges quad_edges(const int *xy8, int hh) {
    QuadEdges E;
    int y_min = 2147483647, y_max = -2147483647, ne = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int i0 = (i + 3) & 3;
        const long long p0x = (long long)xy8[2*i0]*65536, p0y = xy8[2*i0+1], p1x = (long long)xy8[2*i]*65536, p1y = xy8[2*i+1];   // (x * 2^16: negative x)
        E.ev[i] = p0y != p1y;
        const bool up = p0y < p1y;
        E.ey0[i] = (int)(up ? p0y : p1y); E.ey1[i] = (int)(up ? p1y : p0y); E.ex[i] = up ? p0x : p1x;
        E.edx[i] = E.ev[i] ? div_trunc_small(p1x - p0x, p1y - p0y) : 0;      // (|p1x - p0x| <= 2^32 x 2^16, |p1y - p0y| <= 2^32: int coordinates)
        if (E.ev[i]) { y_min = min(y_min, E.ey0[i]); y_max = max(y_max, E.ey1[i]); ne++; }
    }
    const bool any = ne >= 2 && !(y_max < 0 || y_min >= hh);
    E.y_lo = any ? max(y_min, 0) : 0; E.y_hi = any ? min(y_max, hh) : 0;
    return E;
}
// The (at most two) spans of row y, E.y_lo <= y < E.y_hi, clamped to [0, w); an absent span has xa > xb.
struct QuadSpans { int xa[2], xb[2]; };
__device__ __forceinline__ QuadSpans quad_row_spans(const QuadEdges &E, int y, int w) {
    const long long INF = 0x7fffffffffffffffLL;
    long long x0, x1, x2, x3; int na = 0;
    { const bool on = E.ev[0] && E.ey0[0] <= y && y < E.ey1[0]; x0 = on ? E.ex[0] + (long long)(y - E.ey0[0])*E.edx[0] : INF; na += on; }
    { const bool on = E.ev[1] && E.ey0[1] <= y && y < E.ey1[1]; x1 = on ? E.ex[1] + (long long)(y - E.ey0[1])*E.edx[1] : INF; na += on; }
    { const bool on = E.ev[2] && E.ey0[2] <= y && y < E.ey1[2]; x2 = on ? E.ex[2] + (long long)(y - E.ey0[2])*E.edx[2] : INF; na += on; }
    { const bool on = E.ev[3] && E.ey0[3] <= y && y < E.ey1[3]; x3 = on ? E.ex[3] + (long long)(y - E.ey0[3])*E.edx[3] : INF; na += on; }
#define RQ_CX(a_, b_) do { const long long lo_ = a_ < b_ ? a_ : b_, hi_ = a_ < b_ ? b_ : a_; a_ = lo_; b_ = hi_; } while (0)
    RQ_CX(x0, x1); RQ_CX(x2, x3); RQ_CX(x0, x2); RQ_CX(x1, x3); RQ_CX(x1, x2);
#undef RQ_CX
    QuadSpans S;
#pragma unroll
    for (int sp = 0; sp < 2; sp++) {
        S.xa[sp] = 1; S.xb[sp] = 0;
        if (na < 2*sp + 2) continue;
        const long long xl = sp == 0 ? x0 : x2, xr = sp == 0 ? x1 : x3;
        const int xa = (int)((xl + 65535) >> 16), xb = (int)(xr >> 16);
        if (xa < w && xb >= 0) { S.xa[sp] = xa < 0 ? 0 : xa; S.xb[sp] = xb >= w ? w - 1 : xb; }
    }
    return S;
}
// bits b0 .. b1 of the mask (b0 <= b1): a span's bits are contiguous, whole words at a time
__device__ __forceinline__ void mask_set_span(unsigned *mask, int b0, int b1) {
    for (int wd = b0 >> 5; wd <= (b1 >> 5); wd++) {
        unsigned m = 0xffffffffu;
        if (wd == (b0 >> 5)) m &= 0xffffffffu << (b0 & 31);
        if (wd == (b1 >> 5)) m &= 0xffffffffu >> (31 - (b1 & 31));
        atomicOr(&mask[wd], m);
    }
}
// The one rasteriser: cv::fillPoly of one quad (integer corners s_xy, FULL image w x hh), its rows y0 <= y < y1 into a bit mask, pixel (x, y) at bit
// (y - y0) w + x.  A quarter of the threads walks each boundary line and drops the pixels outside the window; the interior takes one thread per row of the
// window.  The caller clears (y1 - y0) w bits and synchronises before and after; for a mask in LDS it chooses y1 - y0 <= MS_MASK_WORDS*32 / w.
// rq_dbg (the -DMID_STAMPS build, tools/mid_stamps.sh): thread 0's cycles after the boundary, the edge slopes and the interior.
__device__ __forceinline__ void raster_quad_rows(unsigned *mask, const int *s_xy, int w, int hh, int y0, int y1, int tid, int nthreads, long long *rq_dbg = nullptr) {
    const long long rq_t0 = rq_dbg ? clock64() : 0;
#define RQ_STAMP(k) do { if (rq_dbg && tid == 0) atomicAdd((unsigned long long *)&rq_dbg[k], (unsigned long long)(clock64() - rq_t0)); } while (0)
    const int per = nthreads >> 2, e = tid/per, li = tid - e*per;
    if (e < 4) {
        const QuadLine L = quad_line(s_xy, e, w, hh);
        if (L.ok)
            for (int i = li; i <= L.major; i += per) {
                long long x, y; quad_line_pixel(L, i, x, y);
                if (x >= 0 && x < w && y >= 0 && y < hh && y >= y0 && y < y1) atomicOr(&mask[((y - y0)*w + x) >> 5], 1u << (((y - y0)*w + x) & 31));
            }
    }
    RQ_STAMP(0);                                                // (boundary lines)
    const QuadEdges E = quad_edges(s_xy, hh);
    RQ_STAMP(1);                                                // (edge slopes)
    for (int y = max(E.y_lo, y0) + tid; y < min(E.y_hi, y1); y += nthreads) {
        const QuadSpans S = quad_row_spans(E, y, w);
#pragma unroll
        for (int sp = 0; sp < 2; sp++)
            if (S.xa[sp] <= S.xb[sp]) mask_set_span(mask, (y - y0)*w + S.xa[sp], (y - y0)*w + S.xb[sp]);
    }
    RQ_STAMP(2);
#undef RQ_STAMP
}
// The whole image's window of the fill: the mask of w hh bits (at most MS_MASK_WORDS*32 in LDS).
__device__ __forceinline__ void raster_quad(unsigned *mask, const int *s_xy, int w, int hh, int tid, int nthreads, long long *rq_dbg = nullptr) {
    raster_quad_rows(mask, s_xy, w, hh, 0, hh, tid, nthreads, rq_dbg);
}
// Point membership of the same fill, without a mask: whether raster_quad sets the bit of pixel (x, y), 0 <= x < w, 0 <= y < hh, for the corners xy8.
// Boundary: is (x, y) pixel il of line e (a line advances one pixel per step along its major axis); interior: the spans of row y.
__device__ __forceinline__ bool quad_covers(const int *xy8, int w, int hh, int x, int y) {
    bool hit = false;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const QuadLine L = quad_line(xy8, e, w, hh);
        const long long il = L.steep ? (y - L.y1)*L.sy : x - L.x1;     // (a line that is not ok has major = 0 at (0, 0))
        if (L.ok && il >= 0 && il <= L.major) {
            long long lx, ly; quad_line_pixel(L, (int)il, lx, ly);
            hit |= lx == x && ly == y;
        }
    }
    const QuadEdges E = quad_edges(xy8, hh);
    if (y >= E.y_lo && y < E.y_hi) {
        const QuadSpans S = quad_row_spans(E, y, w);
        hit |= (S.xa[0] <= x && x <= S.xb[0]) || (S.xa[1] <= x && x <= S.xb[1]);
    }
    return hit;
}
