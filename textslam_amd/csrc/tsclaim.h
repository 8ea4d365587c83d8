// tsclaim.h -- the stateful window searches tracking::SearchForTriangular (src/tracking.cc:1347-1411) and tracking::SearchForInitializ (:1045-1109) and, behind the first,
// GetForTriangular + CheckTriangular (:1413-1497) on the device (tsorb_match_search_claim, tsorb_match_new_points, include/tsorb.h; docs/newpoints_recalled.md is the
// arithmetic).  The point is tstexttheta.h's tt_triangulate_between; the walks are tsorb.hip's match_walk.  Three launches, no workgroup waits for another:
//   k_claim_walk    a wave per query: match_walk over the context's grid, eligible features only.  The first CL_ROW candidates (index, distance) of every query stay in
//                   device scratch in the reference's order, with the number there were.
//   k_claim_chain   ONE workgroup, the reference's loop over the queries in order.  vMatchDist lives in LDS as 16 bits a feature (0 = not eligible: hidden from every
//                   distance; CL_FREE = INT_MAX).  Wave 0 is the chain: a step puts the query's candidates on its lanes, 64 at a time, reads vMatchDist, keeps per lane
//                   the smallest (distance << 16 | position in the list) key and the second smallest distance, merges the lanes by a butterfly and decides.  The position
//                   in the key is the order-preserving part: the first minimum in CANDIDATE order.  Waves 1 .. 3 stage the next CL_BLK queries' lists from scratch into
//                   the other half of an LDS buffer meanwhile, so a step never waits for global memory; one barrier per CL_BLK steps.  A query with more than CL_ROW
//                   candidates is walked again by wave 0 with the vMatchDist test inside the walk: never an answer from a cut list.  vMatchIdx21 is written to scratch
//                   as the chain goes (stores only) and turned into vMatchIdx12 at the end: the two are inverse to each other at every step of the reference.
//   k_claim_points  a thread per query with a match: cv::triangulatePoints between Trw and Tcw, the float division, CheckTriangular.
// Everything that decides anything is __host__ __device__: tests/cxx/new_points_host.hip runs it on the CPU.  fp64, one rounding per operation, no contraction.
#pragma once
#pragma clang fp contract(off)
#include "tstexttheta.h"

#define CL_T     256                 /* threads of k_claim_chain and k_claim_points; k_claim_walk: four waves = four queries */
#define CL_ROW   256                 /* candidates of a query kept in scratch (a 96-px window of one octave in a 1000-feature frame holds about 35, the initializer's 100-px window over 1000 octave-0 features 120 - 175; with a row of 128 its re-walks made that call 6.7 ms) */
#define CL_BLK   8                   /* queries staged per block: 2 x CL_BLK x CL_ROW dwords of LDS */
#define CL_FREE  0xffff              /* vMatchDist = INT_MAX */
#define CL_NONE  0x7fffffff          /* key of "no candidate": its distance field (key >> 16 = 0x7fff) is above every th_low */
#define CL_NO2   0x7fff              /* "no runner-up" while merging; INT_MAX in the acceptance test */

struct ClaimDev {
    int nq, n2, th_low, use_ratio; double ratio;
    const float *qxy, *qr; const int32_t *qlev; const uint8_t *qdesc, *elig;
    int32_t *row_idx, *row_dist, *row_cnt;                                 // scratch: [nq][CL_ROW], [nq][CL_ROW], [nq]
    int32_t *own;                                                          // scratch: [n2] vMatchIdx21
    int32_t *match12, *match_dist, *count;                                 // [nq], [nq], { n_match, n_good }
    const float *q_px; double Trw[12], Tcw[12], K[4]; int th_reproj; float *p3d; uint8_t *good;       // k_claim_points
};

// ---- the chain's decisions
// `if(vMatchDist[i2]<=dist) continue;` on the 16-bit state: 0 hides the feature from every distance, CL_FREE from none (a distance is at most 256)
__host__ __device__ __forceinline__ bool cl_hidden(int md, int d) { return md <= d; }
// what a candidate offers to the step: its key, or none when it is hidden
__host__ __device__ __forceinline__ int cl_offer(int md, int d, int pos) { return cl_hidden(md, d) ? CL_NONE : ((d << 16) | pos); }
// (key, second): the smallest key (the first position of the smallest distance) and the second smallest distance of a multiset, merged with another's
__host__ __device__ __forceinline__ void cl_merge(int &k1, int &s2, int ok, int os) {
    const int hi = (k1 > ok ? k1 : ok) >> 16, lo = s2 < os ? s2 : os;
    k1 = k1 < ok ? k1 : ok; s2 = lo < hi ? lo : hi;
}
// `bestDist<=TH_LOW` and, for SearchForInitializ, `bestDist<(double)bestDist2*0.9` as written; best = the key's distance
__host__ __device__ __forceinline__ bool cl_accept(int k1, int s2, int th_low, int use_ratio, double ratio, int &best) {
    best = k1 >> 16;
    const int second = s2 == CL_NO2 ? 2147483647 : s2;
    return best <= th_low && (!use_ratio || (double)best < (double)second*ratio);
}

// ---- GetForTriangular's point and CheckTriangular
// CheckTriangular (tracking.cc:1461-1497) of one point as written: no depth test, and a NaN error passes both `>` tests
__host__ __device__ inline bool cl_check(const double Trw[12], const double Tcw[12], const double K[4], const float X[3], const float *pt1, const float *pt2, int th_reproj) {
    const double p0 = (double)X[0], p1 = (double)X[1], p2 = (double)X[2], fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    if (!__builtin_isfinite(p0) || !__builtin_isfinite(p1) || !__builtin_isfinite(p2)) return false;
    double ref[3], cur[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {                                          // Eigen's fixed-size product left to right, then the translation
        ref[r] = ((Trw[4*r]*p0 + Trw[4*r + 1]*p1) + Trw[4*r + 2]*p2) + Trw[4*r + 3];
        cur[r] = ((Tcw[4*r]*p0 + Tcw[4*r + 1]*p1) + Tcw[4*r + 2]*p2) + Tcw[4*r + 3]; }
    const float th = (float)th_reproj;
    const double u1 = (fx*ref[0])/ref[2] + cx, v1 = (fy*ref[1])/ref[2] + cy;
    if (u1 < 0 || v1 < 0) return false;
    const double a1 = u1 - (double)pt1[0], b1 = v1 - (double)pt1[1];
    const float e1 = (float)(a1*a1 + b1*b1);
    if (e1 > th) return false;
    const double u2 = (fx*cur[0])/cur[2] + cx, v2 = (fy*cur[1])/cur[2] + cy;
    const double a2 = u2 - (double)pt2[0], b2 = v2 - (double)pt2[1];
    const float e2 = (float)(a2*a2 + b2*b2);
    if (e2 > th) return false;
    return true;
}
// one match: the point between the cameras Trw (pixel pt1) and Tcw (pixel pt2), and whether CheckTriangular keeps it
__host__ __device__ inline bool cl_new_point(const double Trw[12], const double Tcw[12], const double K[4], const float *pt1, const float *pt2, int th_reproj, float X[3]) {
    double rho;
    tt_triangulate_between(Trw, Tcw, K, pt1, pt2, X, rho);
    return cl_check(Trw, Tcw, K, X, pt1, pt2, th_reproj);
}

#ifndef TSCLAIM_HOST_ONLY                                             /* tests/cxx/new_points_host.hip: the functions above only */
// ---- the walks' further tests (match_walk's Keep)
struct ClElig { const uint8_t *elig; __device__ __forceinline__ bool operator()(int i, int) const { return !elig || elig[i] != 0; } };
struct ClOpen { const unsigned short *md; __device__ __forceinline__ bool operator()(int i, int d) const { return !cl_hidden((int)md[i], d); } };

__device__ __forceinline__ void cl_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void cl_query(const ClaimDev &D, int q, uint32_t (&qd)[8], float &x, float &y, float &r, int &l0, int &l1) {
#pragma unroll
    for (int k = 0; k < 8; k++) qd[k] = ((const uint32_t *)D.qdesc)[8*(size_t)q + k];
    x = D.qxy[2*(size_t)q]; y = D.qxy[2*(size_t)q + 1]; r = D.qr[q]; l0 = D.qlev ? D.qlev[2*(size_t)q] : -1; l1 = D.qlev ? D.qlev[2*(size_t)q + 1] : -1;
}

__global__ __launch_bounds__(256) void k_claim_walk(MatchGrid G, ClaimDev D) {
    __shared__ int s_inc[4][64], s_o0[4][64], s_best[4][3];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x*4 + wv;
    if (q >= D.nq) return;                                                 // (a whole wave)
    uint32_t qd[8]; float x, y, r; int l0, l1;
    cl_query(D, q, qd, x, y, r, l0, l1);
    const ClElig keep = { D.elig };
    match_walk(G, lane, s_inc[wv], s_o0[wv], x, y, r, l0, l1, qd, CL_ROW, D.row_idx + (size_t)q*CL_ROW, D.row_dist + (size_t)q*CL_ROW, D.row_cnt + q,
               &s_best[wv][0], &s_best[wv][1], &s_best[wv][2], keep);
}

// waves 1 .. 3: block b's lists from scratch into buffer `buf`, every slot of every row (the unused ones hold -1 and are never read: a step stops at the row's count)
__device__ __forceinline__ void cl_stage(const ClaimDev &D, int b, int (*s_row)[CL_ROW], int *s_cnt, int t) {
    const int q0 = b*CL_BLK, nt = CL_T - 64;
    if (t < CL_BLK) s_cnt[t] = q0 + t < D.nq ? D.row_cnt[q0 + t] : 0;
#pragma unroll
    for (int u = 0; u < (CL_BLK*CL_ROW + nt - 1)/nt; u++) {
        const int e = t + u*nt, k = e/CL_ROW, p = e - k*CL_ROW;
        if (e < CL_BLK*CL_ROW && q0 + k < D.nq) { const size_t g = (size_t)(q0 + k)*CL_ROW + p; s_row[k][p] = (D.row_dist[g] << 16) | (D.row_idx[g] & 0xffff); }
    }
}

__global__ __launch_bounds__(CL_T) void k_claim_chain(MatchGrid G, ClaimDev D) {
    extern __shared__ unsigned short s_md[];                               // [n2] vMatchDist
    __shared__ int s_row[2][CL_BLK][CL_ROW];
    __shared__ int s_cnt[2][CL_BLK];
    __shared__ int s_inc[64], s_o0[64], s_w[4], s_n;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nq = D.nq, n2 = D.n2, nb = (nq + CL_BLK - 1)/CL_BLK;
    for (int i = tid; i < n2; i += CL_T) { s_md[i] = (D.elig && !D.elig[i]) ? 0 : CL_FREE; D.own[i] = -1; }
    for (int q = tid; q < nq; q += CL_T) { D.match12[q] = -1; D.match_dist[q] = -1; }
    if (tid == 0) { s_n = 0; D.count[1] = 0; }
    if (wv > 0) cl_stage(D, 0, s_row[0], s_cnt[0], tid - 64);
    __syncthreads();
    for (int b = 0; b < nb; b++) {
        const int buf = b & 1;
        if (wv > 0) { if (b + 1 < nb) cl_stage(D, b + 1, s_row[buf ^ 1], s_cnt[buf ^ 1], tid - 64); }
        else {
            const int kn = min(CL_BLK, nq - b*CL_BLK);
            for (int k = 0; k < kn; k++) {                                  // the reference's loop over i1
                const int q = b*CL_BLK + k, cnt = __builtin_amdgcn_readfirstlane(s_cnt[buf][k]);
                int k1 = CL_NONE, s2 = CL_NO2, i2 = -1;
                if (cnt <= CL_ROW) {                                       // (uniform over the wave)
                    for (int c0 = 0; c0 < cnt; c0 += 64) { const int pos = c0 + lane;
                        if (pos < cnt) { const int e = s_row[buf][k][pos]; cl_merge(k1, s2, cl_offer((int)s_md[e & 0xffff], e >> 16, pos), CL_NO2); } }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) { const int ok = __shfl_xor(k1, o, 64), os = __shfl_xor(s2, o, 64); cl_merge(k1, s2, ok, os); }
                    if (k1 != CL_NONE) i2 = s_row[buf][k][k1 & 0xffff] & 0xffff;
                } else {                                                   // more candidates than a row holds: the walk again, vMatchDist tested inside it
                    uint32_t qd[8]; float x, y, r; int l0, l1;
                    cl_query(D, q, qd, x, y, r, l0, l1);
                    const ClOpen keep = { s_md };
                    match_walk(G, lane, s_inc, s_o0, x, y, r, l0, l1, qd, 0, (int *)nullptr, (int *)nullptr, &s_w[0], &s_w[1], &s_w[2], &s_w[3], keep);
                    cl_wave_sync();
                    const int bd = s_w[2], bd2 = s_w[3];
                    if (bd != 2147483647) { k1 = bd << 16; i2 = s_w[1]; s2 = bd2 == 2147483647 ? CL_NO2 : bd2; }
                    cl_wave_sync();                                        // (the next such query writes s_w again)
                }
                int best;
                if (cl_accept(k1, s2, D.th_low, D.use_ratio, D.ratio, best) && lane == 0) { s_md[i2] = (unsigned short)best; D.own[i2] = q; }
            }
        }
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < n2; i += CL_T) { const int o = D.own[i];        // vMatchIdx12 from vMatchIdx21
        if (o >= 0) { D.match12[o] = i; D.match_dist[o] = (int)s_md[i]; atomicAdd(&s_n, 1); } }
    __syncthreads();
    if (tid == 0) D.count[0] = s_n;
}

__global__ __launch_bounds__(CL_T) void k_claim_points(MatchGrid G, ClaimDev D) {
    const int q = blockIdx.x*CL_T + threadIdx.x;
    bool g = false;
    if (q < D.nq) {
        const int m = D.match12[q];
        float X[3] = { 0.f, 0.f, 0.f };
        if (m >= 0) { const float pt2[2] = { G.kp[6*(size_t)m], G.kp[6*(size_t)m + 1] };
            g = cl_new_point(D.Trw, D.Tcw, D.K, D.q_px + 2*(size_t)q, pt2, D.th_reproj, X); }
        D.p3d[3*(size_t)q] = X[0]; D.p3d[3*(size_t)q + 1] = X[1]; D.p3d[3*(size_t)q + 2] = X[2]; D.good[q] = g ? 1 : 0;
    }
    const unsigned long long gm = __ballot(g);
    if ((threadIdx.x & 63) == 0 && gm) atomicAdd(&D.count[1], __popcll(gm));
}
#endif
