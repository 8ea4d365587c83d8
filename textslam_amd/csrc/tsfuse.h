// tsfuse.h -- the rest of frame::FeatExtract and frame::FeatFusion (src/frame.cc:234-325) on the device: tool::BoundFeatDele_T's boundary test on the raw text
// features k_cvo_describe left in device scratch (src/tool.cc:456-508), and the concatenation of the resident frame's scene features with the surviving text
// features into the set tsorb_match_* searches.  docs/pointpolygon_recalled.md is cv::pointPolygonTest; fuse_point_in_polygon below is that document and the only
// statement of the test: the kernels, tests/cxx/fuse_frame_from_cxx.cpp --host and the g++ program of tests/test_fuse_frame_ref.py all call it (this part of the
// file compiles with plain g++).
//
// The launches of a call, behind the 13 of the text extraction (tscvorb.h):
//   k_fuse_keep     a workgroup per detection: its raw rows 256 at a time, the two polygon tests per lane, the kept rows' raw indices in raw order (ballot inside
//                   a wave, the four waves' counts through LDS, a running prefix across the chunks) and their count
//   k_fuse_offsets  one workgroup: the exclusive scan of the kept counts -> text_off, n_out, the two capacity verdicts
//   k_fuse_gather   8 lanes per fused row: 24 + 32 bytes from the scene outputs or the raw text rows into the device set the grid reads and into the pinned block;
//                   obj and src beside them
// No workgroup waits for another; every loop is bounded by a size of the call (cap_text, n_dete, cap); every index is below the capacity of the array it reads or
// writes: a raw row below min(raw, cap_text), a fused row below min(n, cap), a scene row below the resident frame's count (which tsorb_run caps at its own cap).
#pragma once
#include <stdint.h>
#include <float.h>

#if defined(__HIPCC__)
#define TSFUSE_HD __host__ __device__
#else
#define TSFUSE_HD
#endif

// cv::Point(double, double): truncation towards zero; a value no int holds becomes INT32_MIN (what the x86 conversion gives), so that host and tests agree
TSFUSE_HD static inline int fuse_trunc(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (int)(-2147483647 - 1); }

// tool::GetNewDeteBox + tool::vV2vP: the quad's corners moved by win (negative: inwards for corners in the order top-left, top-right, bottom-right, bottom-left)
TSFUSE_HD static inline void fuse_shrunk_quad(const double *quad /*[4][2]*/, double win, int *poly /*[4][2]*/) {
    poly[0] = fuse_trunc(quad[0] - win); poly[1] = fuse_trunc(quad[1] - win);
    poly[2] = fuse_trunc(quad[2] + win); poly[3] = fuse_trunc(quad[3] - win);
    poly[4] = fuse_trunc(quad[4] + win); poly[5] = fuse_trunc(quad[5] + win);
    poly[6] = fuse_trunc(quad[6] - win); poly[7] = fuse_trunc(quad[7] + win);
}
// tool::GetbbDeteBox + tool::vV2vP: bbox = vTextDeteMin x, y, vTextDeteMax x, y
TSFUSE_HD static inline void fuse_bbox_quad(const double *bbox /*[4]*/, int *poly /*[4][2]*/) {
    const int x0 = fuse_trunc(bbox[0]), y0 = fuse_trunc(bbox[1]), x1 = fuse_trunc(bbox[2]), y1 = fuse_trunc(bbox[3]);
    poly[0] = x0; poly[1] = y0; poly[2] = x1; poly[3] = y0; poly[4] = x1; poly[5] = y1; poly[6] = x0; poly[7] = y1;
}

// tool::CheckPtsIn: cv::pointPolygonTest(contour of n int points, Point2f(px, py), measureDist = true) > 0 (docs/pointpolygon_recalled.md).  The differences are
// float subtractions widened to double; every product that is added is exact in double, so a contracted multiply-add rounds as the separate operations do.
TSFUSE_HD static inline bool fuse_point_in_polygon(const int *poly /*[n][2]*/, int n, float px, float py) {
    if (n <= 0) return false;
    double min_num = FLT_MAX, min_den = 1.0;
    int counter = 0;
    float vx = (float)poly[2*(n - 1)], vy = (float)poly[2*(n - 1) + 1];
    for (int i = 0; i < n; i++) {
        const float v0x = vx, v0y = vy;
        vx = (float)poly[2*i]; vy = (float)poly[2*i + 1];
        const double dx = (double)(vx - v0x), dy = (double)(vy - v0y), dx1 = (double)(px - v0x), dy1 = (double)(py - v0y), dx2 = (double)(px - vx), dy2 = (double)(py - vy);
        double num, den = 1.0;
        if (dx1*dx + dy1*dy <= 0) num = dx1*dx1 + dy1*dy1;
        else if (dx2*dx + dy2*dy >= 0) num = dx2*dx2 + dy2*dy2;
        else { num = dy1*dx - dx1*dy; num *= num; den = dx*dx + dy*dy; }
        if (num*min_den < min_num*den) { min_num = num; min_den = den; if (min_num == 0) break; }
        if ((v0y <= py && vy <= py) || (v0y > py && vy > py)) continue;
        double t = dy1*dx - dx1*dy;
        if (dy < 0) t = -t;
        counter += t > 0;
    }
    return min_num != 0 && (counter & 1);                               // sqrt(min_num/min_den), negated when the counter is even, > 0
}
// tool.cc:484: kept iff inside the shrunk quad and inside the bounding box; polys = [shrunk | bb], 16 ints
TSFUSE_HD static inline bool fuse_keep_point(const int *polys, float x, float y) { return fuse_point_in_polygon(polys, 4, x, y) && fuse_point_in_polygon(polys + 8, 4, x, y); }

#if defined(__HIPCC__)
struct FuseDev {
    int nd, cap_text, cap;
    const int *poly;                                    // (pinned) [nd][16] shrunk quad, bounding box
    const int *raw_cnt; const float *raw_kp; const uint8_t *raw_desc;      // what the text extraction wrote: [nd], [nd][cap_text][6], [nd][cap_text][32]
    const int *sc_cnt; const float *sc_kp; const uint8_t *sc_desc;         // the resident frame's count, keypoints, descriptors
    int *keep_idx, *keep_cnt;                           // [nd][cap_text] raw indices of the kept rows, [nd]
    int *head;                                          // [nd + 1] text_off, [2] n_out, [2] verdicts: every detection fits cap_text, n fits cap
    float *set_kp; uint8_t *set_desc;                   // [cap][6], [cap][32]: the set the grid reads
    int *o_head, *o_raw, *o_obj, *o_src; float *o_kp; uint8_t *o_desc;     // (pinned) head as above, [nd], [cap], [cap], [cap][6], [cap][32]
};

// grid (nd), 256 lanes
__global__ __launch_bounds__(256) void k_fuse_keep(FuseDev F) {
    __shared__ int s_poly[16], s_wave[4];
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 16) s_poly[tid] = F.poly[16*(size_t)d + tid];
    const int raw = F.raw_cnt[d], rows = raw > F.cap_text ? 0 : raw;           // (a detection that does not fit has no rows: the call fails in k_fuse_offsets)
    __syncthreads();
    int base = 0;
    for (int c = 0; c < rows; c += 256) {                                     // (rows <= cap_text)
        const int i = c + tid;
        bool keep = false;
        if (i < rows) { const float *k = F.raw_kp + ((size_t)d*F.cap_text + i)*6; keep = fuse_keep_point(s_poly, k[0], k[1]); }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) { const int n = s_wave[w]; before += w < wave ? n : 0; all += n; }
        if (keep) F.keep_idx[(size_t)d*F.cap_text + base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;      // (a place below the rows seen so far: < cap_text)
        base += all;
        __syncthreads();
    }
    if (tid == 0) F.keep_cnt[d] = base;
}

// grid (1), 256 lanes: detections 256 at a time
__global__ __launch_bounds__(256) void k_fuse_offsets(FuseDev F) {
    __shared__ int s[256], s_fit;
    const int tid = threadIdx.x, n_scene = F.sc_cnt[0];
    if (tid == 0) s_fit = 1;
    __syncthreads();
    int base = n_scene;
    for (int c = 0; c < F.nd; c += 256) {
        const int d = c + tid, v = d < F.nd ? F.keep_cnt[d] : 0;
        if (d < F.nd) { const int raw = F.raw_cnt[d]; F.o_raw[d] = raw; if (raw > F.cap_text) s_fit = 0; }
        s[tid] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) { const int a = tid >= o ? s[tid - o] : 0; __syncthreads(); s[tid] += a; __syncthreads(); }
        if (d < F.nd) { const int off = base + s[tid] - v; F.head[d] = off; F.o_head[d] = off; }
        base += s[255];
        __syncthreads();
    }
    if (tid == 0) { const int fit = s_fit, ok = base <= F.cap;
        F.head[F.nd] = base; F.head[F.nd + 1] = n_scene; F.head[F.nd + 2] = base; F.head[F.nd + 3] = fit; F.head[F.nd + 4] = ok;
        F.o_head[F.nd] = base; F.o_head[F.nd + 1] = n_scene; F.o_head[F.nd + 2] = base; F.o_head[F.nd + 3] = fit; F.o_head[F.nd + 4] = ok; }
}

// grid (ceil(8 cap / 256)), 8 lanes per fused row; nothing is written when a capacity was too small
__global__ __launch_bounds__(256) void k_fuse_gather(FuseDev F) {
    const int row = (int)((blockIdx.x*256u + threadIdx.x) >> 3), sub = threadIdx.x & 7;
    const int *head = F.head + F.nd;                                          // n, n_scene, n, fit, ok
    if (!head[3] || !head[4]) return;
    const int n = head[0], n_scene = head[1];
    if (row >= n || row >= F.cap) return;
    const uint32_t *kp, *de; int obj = -1, src = row;
    if (row < n_scene) { kp = (const uint32_t *)(F.sc_kp + (size_t)row*6); de = (const uint32_t *)(F.sc_desc + (size_t)row*32); }
    else {
        int lo = 0, hi = F.nd;                                                // the last detection whose first row is <= row: text_off never decreases, text_off[nd] = n > row
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (F.head[mid] <= row) lo = mid; else hi = mid; }
        obj = lo; src = F.keep_idx[(size_t)lo*F.cap_text + (row - F.head[lo])];
        kp = (const uint32_t *)(F.raw_kp + ((size_t)lo*F.cap_text + src)*6); de = (const uint32_t *)(F.raw_desc + ((size_t)lo*F.cap_text + src)*32);
    }
    const uint32_t b = de[sub];
    ((uint32_t *)(F.set_desc + (size_t)row*32))[sub] = b; ((uint32_t *)(F.o_desc + (size_t)row*32))[sub] = b;
    if (sub < 6) { const uint32_t a = kp[sub]; ((uint32_t *)(F.set_kp + (size_t)row*6))[sub] = a; ((uint32_t *)(F.o_kp + (size_t)row*6))[sub] = a; }
    if (sub == 6) F.o_obj[row] = obj;
    if (sub == 7) F.o_src[row] = src;
}
#endif
