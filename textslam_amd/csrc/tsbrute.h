// tsbrute.h -- all-pairs descriptor matching of loop closing (loopClosing::SearchMatch, src/loopClosing.cc:738-925), included by tsorb.hip.
//   k_brute_text / k_brute_good  <- loopClosing::FeatureMatch_brute(.., USETHRESH = true) (:1491-1519) for every matched text pair of every loop candidate:
//                                   cv::BFMatcher(NORM_HAMMING)::match (docs/bfmatcher_recalled.md) and the max(2 min_dist, 30.0) cut
//   k_brute_scene                <- loopClosing::SearchMatch_Other (:823-925): the sequential claim scan over the current keyframe's features, one
//                                   workgroup per loop candidate, the text label images answered by quad_covers (tsraster.h) instead of being painted
// Every loop below is bounded by a feature count, a box count or a constant; no workgroup reads what another one wrote in the same launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tsraster.h"

#define BR_T      256                 /* threads per workgroup of every kernel here */
#define BR_SLOTS  4                   /* candidate features a thread of k_brute_scene keeps in registers: i2 = tid + BR_T k, k < BR_SLOTS */
#define BR_CHUNK  (BR_T/2)            /* descriptors of the current keyframe staged in LDS at a time: 16 bytes a thread */
#define BR_NONE   0x7fffffff          /* packed key of "no candidate": its distance field (key >> 16 = 0x7fff) is above every th_low */
#define BR_NO2    0x7fff              /* "no runner-up" while reducing; INT_MAX in the acceptance test */

__device__ __forceinline__ int br_hamming(const uint32_t *a, const uint32_t *b) {
    int d = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) d += __popc(a[w] ^ b[w]);
    return d;
}

// ------------------------------------------------------------------ text pairs
// A tile = up to BR_T queries of one pair (tile[b] = {pair, first query row}); a thread owns a query and walks the pair's set 2 in index order through LDS
// (BR_T rows at a time, every thread reading the same row: a broadcast), strict < : the first index of the minimum.  The pair's minimum distance is an
// atomicMin on pmin[pair] (set to INT_MAX by the host before the launch); k_brute_good turns it into the flags in a launch of its own, so no workgroup waits.
struct BruteText {
    const int2 *tile; const int *off1, *off2; const uint8_t *desc1, *desc2;
    int *train, *dist, *pmin; uint8_t *good;
};
__global__ __launch_bounds__(BR_T) void k_brute_text(BruteText B) {
    __shared__ uint32_t s_d[BR_T][8];
    const int tid = threadIdx.x, p = B.tile[blockIdx.x].x, q = B.tile[blockIdx.x].y + tid;
    const bool active = q < B.off1[p + 1];
    const int o2 = B.off2[p], n2 = B.off2[p + 1] - o2;
    uint32_t qd[8];
#pragma unroll
    for (int w = 0; w < 8; w++) qd[w] = active ? ((const uint32_t *)B.desc1)[8*(size_t)q + w] : 0u;
    int best = 2147483647, bi = -1;
    for (int j0 = 0; j0 < n2; j0 += BR_T) {
        const int nj = min(BR_T, n2 - j0);
        __syncthreads();
        if (tid < nj) {
#pragma unroll
            for (int w = 0; w < 8; w++) s_d[tid][w] = ((const uint32_t *)B.desc2)[8*(size_t)(o2 + j0 + tid) + w];
        }
        __syncthreads();
        if (active)
            for (int j = 0; j < nj; j++) { const int d = br_hamming(qd, s_d[j]); if (d < best) { best = d; bi = j0 + j; } }
    }
    if (active) { B.train[q] = bi; B.dist[q] = best; atomicMin(&B.pmin[p], best); }
}
__global__ __launch_bounds__(BR_T) void k_brute_good(BruteText B) {
    const int p = B.tile[blockIdx.x].x, q = B.tile[blockIdx.x].y + threadIdx.x;
    if (q >= B.off1[p + 1]) return;
    const double cut = fmax(2.0*(double)B.pmin[p], 30.0);                       // max(2*min_dist, 30.0), min_dist a double of the integer
    B.good[q] = (B.off2[p + 1] > B.off2[p] && (double)B.dist[q] < cut) ? 1 : 0;      // (an empty set 2: no match, never good)
}

// ------------------------------------------------------------------ scene features against a loop candidate's
struct BruteScene {
    int w, h, n1, th_low; double ratio;
    const float *xy1; const uint8_t *desc1, *has3d1;
    const int *off2; const float *xy2; const uint8_t *desc2, *has3d2;
    const int *qoff, *quad_cur, *quad_can;                                      // corners already truncated to int (cv::Point(double, double))
    int *md, *own;                                                              // [off2[n_cand]]: vMatchDist (-1 = not eligible) and vMatchIdx21
    int *match12, *n_match;
};
// label >= 0 at the rounded pixel of (x, y) in an image that has the boxes [q0, q1) filled; outside the image: not covered
__device__ bool br_covered(const float *xy, const int *quad, int q0, int q1, int w, int h) {
    const float rx = roundf(xy[0]), ry = roundf(xy[1]);
    if (!(rx >= 0.f && rx < (float)w && ry >= 0.f && ry < (float)h)) return false;
    const int px = (int)rx, py = (int)ry;
    bool hit = false;
    for (int q = q0; q < q1 && !hit; q++) {
        int c8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) c8[k] = quad[8*(size_t)q + k];
        hit = quad_covers(c8, w, h, px, py);
    }
    return hit;
}
// the next set bit of the eligibility mask after position i (-1: from the start); -1 when there is none.  Every thread reads the same words.
__device__ __forceinline__ int br_next(const unsigned *mask, int nw, int i) {
    const int s = i + 1;
    for (int wd = s >> 5; wd < nw; wd++) {
        unsigned bits = mask[wd];
        if (wd == (s >> 5)) bits &= 0xffffffffu << (s & 31);
        if (bits) return wd*32 + __ffs((int)bits) - 1;
    }
    return -1;
}
// (key, second): the smallest packed key (dist << 16 | i2: the first index of the minimum distance) and the second smallest distance of a multiset
__device__ __forceinline__ void br_merge(int &k1, int &s2, int ok, int os) {
    const int hi = max(k1, ok) >> 16;
    k1 = min(k1, ok); s2 = min(min(s2, os), hi);
}
// One workgroup per candidate.  Phase 1: which features of the current keyframe are eligible for THIS candidate (a bit mask in LDS) and which of the candidate's
// (md = INT_MAX, or -1 = never passes the reference's vMatchDist[i2] <= dist filter).  Phase 2: the reference's chain over i1 in index order; a step is an
// arg-min over the candidate's features -- the first BR_T*BR_SLOTS of them in registers (descriptor, vMatchDist, vMatchIdx21), the rest read from memory --
// reduced in the wave and then over the waves through LDS, double-buffered so that a step needs one barrier.  vMatchIdx12 is written once at the end from
// vMatchIdx21: the two are inverse to each other at every step of the reference (a steal resets the previous owner).
__global__ __launch_bounds__(BR_T) void k_brute_scene(BruteScene S) {
    __shared__ unsigned s_el[TSORB_BRUTE_MAX_FEAT/32];
    __shared__ int s_red[2][BR_T/64][2];
    __shared__ int s_cnt[BR_T/64];
    __shared__ uint4 s_cur[BR_T];                                                                     // BR_CHUNK descriptors of the current keyframe
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = blockIdx.x, n1 = S.n1;
    const int o2 = S.off2[c], n2 = S.off2[c + 1] - o2, q0 = S.qoff[c], q1 = S.qoff[c + 1];
    const int nw = (n1 + 31) >> 5;
    int *m12 = S.match12 + (size_t)c*n1;
    for (int wd = tid; wd < nw; wd += BR_T) s_el[wd] = 0u;
    for (int i = tid; i < n1; i += BR_T) m12[i] = -1;
    __syncthreads();
    for (int i = tid; i < n1; i += BR_T)
        if (S.has3d1[i] && !br_covered(S.xy1 + 2*(size_t)i, S.quad_cur, q0, q1, S.w, S.h)) atomicOr(&s_el[i >> 5], 1u << (i & 31));
    for (int i = tid; i < n2; i += BR_T) {
        const bool e = S.has3d2[o2 + i] && !br_covered(S.xy2 + 2*(size_t)(o2 + i), S.quad_can, q0, q1, S.w, S.h);
        S.md[o2 + i] = e ? 2147483647 : -1; S.own[o2 + i] = -1;
    }
    __syncthreads();
    uint32_t d2[BR_SLOTS][8]; int md[BR_SLOTS], ow[BR_SLOTS];
#pragma unroll
    for (int k = 0; k < BR_SLOTS; k++) {
        const int i2 = tid + BR_T*k; const bool in = i2 < n2;
        md[k] = in ? S.md[o2 + i2] : -1; ow[k] = -1;                                                  // (written above by this same thread)
#pragma unroll
        for (int w = 0; w < 8; w++) d2[k][w] = in ? ((const uint32_t *)S.desc2)[8*(size_t)(o2 + i2) + w] : 0u;
    }
    int par = 0;
    for (int base = 0; base < n1; base += BR_CHUNK) {                                                 // (at most n1 steps in all: i1 strictly increases)
        // the current keyframe's descriptors of the next BR_CHUNK indices through LDS, 16 bytes a thread: a step then reads its descriptor as a broadcast and
        // no step waits for global memory (a load per step, even issued a step ahead, was waited for at once: 0.95 us a step)
        const int nwc = min(nw, (base + BR_CHUNK) >> 5);
        int i1 = br_next(s_el, nwc, base - 1);
        if (i1 < 0) continue;                                                                         // (uniform: the mask is the same for every thread)
        if (2*(size_t)base + tid < 2*(size_t)n1) s_cur[tid] = ((const uint4 *)S.desc1)[2*(size_t)base + tid];
        __syncthreads();
        while (i1 >= 0) {
            const uint4 ca = s_cur[2*(i1 - base)], cb = s_cur[2*(i1 - base) + 1];
            const uint32_t cur[8] = { ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w };
            int k1 = BR_NONE, s2 = BR_NO2;
#pragma unroll
            for (int k = 0; k < BR_SLOTS; k++) {
                const int d = br_hamming(cur, d2[k]);
                if (!(md[k] <= d)) br_merge(k1, s2, (d << 16) | (tid + BR_T*k), BR_NO2);
            }
            for (int i2 = tid + BR_T*BR_SLOTS; i2 < n2; i2 += BR_T) {                                     // beyond the registers
                const int m = S.md[o2 + i2];
                if (m < 0) continue;
                uint32_t f[8];
#pragma unroll
                for (int w = 0; w < 8; w++) f[w] = ((const uint32_t *)S.desc2)[8*(size_t)(o2 + i2) + w];
                const int d = br_hamming(cur, f);
                if (!(m <= d)) br_merge(k1, s2, (d << 16) | i2, BR_NO2);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const int ok = __shfl_xor(k1, o, 64), os = __shfl_xor(s2, o, 64); br_merge(k1, s2, ok, os); }
            if (lane == 0) { s_red[par][wv][0] = k1; s_red[par][wv][1] = s2; }
            __syncthreads();
            k1 = s_red[par][0][0]; s2 = s_red[par][0][1];
#pragma unroll
            for (int v = 1; v < BR_T/64; v++) br_merge(k1, s2, s_red[par][v][0], s_red[par][v][1]);
            const int bestDist = k1 >> 16, bestIdx2 = k1 & 0xffff, bestDist2 = s2 == BR_NO2 ? 2147483647 : s2;
            if (bestDist <= S.th_low && (double)bestDist < (double)bestDist2*S.ratio && (bestIdx2 & (BR_T - 1)) == tid) {
                const int slot = bestIdx2/BR_T;                                                           // this thread holds bestIdx2
                if (slot < BR_SLOTS) {
#pragma unroll
                    for (int k = 0; k < BR_SLOTS; k++) if (k == slot) { md[k] = bestDist; ow[k] = i1; }
                } else { S.md[o2 + bestIdx2] = bestDist; S.own[o2 + bestIdx2] = i1; }
            }
            i1 = br_next(s_el, nwc, i1); par ^= 1;
        }
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < BR_SLOTS; k++) if (ow[k] >= 0) { m12[ow[k]] = tid + BR_T*k; cnt++; }
    for (int i2 = tid + BR_T*BR_SLOTS; i2 < n2; i2 += BR_T) { const int o = S.own[o2 + i2]; if (o >= 0) { m12[o] = i2; cnt++; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int v = 0; v < BR_T/64; v++) t += s_cnt[v]; S.n_match[c] = t; }
}
