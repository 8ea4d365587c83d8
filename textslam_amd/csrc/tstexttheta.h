// tstexttheta.h -- tracking::GetTextTheta / SolveTheta and initializer::CalculateTextTheta on the device (tsorb_match_text_theta_ransac, include/tsorb.h;
// docs/texttheta_recalled.md is the arithmetic).  Three launches, no workgroup waits for another:
//   k_tt_rho      one thread per feature.  rho given: it is copied and the point is zero.  Otherwise cv::triangulatePoints between [I | 0] and Tcr: the 4 x 4 in
//                 double, its null vector by the one-sided iteration on the four columns in fp64 in registers (a lane turning until ITS matrix has converged), the
//                 4-vector rounded to float, the division by its last entry as a float reciprocal and a float product per entry, rho = 1.0/(double)z.
//   k_tt_score    a workgroup per (plane, block of 256 hypotheses), a lane per hypothesis.  The plane's rays, rho and targets are staged once in LDS as doubles
//                 (40 bytes a feature); the lane solves its triple's theta in registers and walks the features in index order, every lane reading the same LDS
//                 address: the reference's summation order, no cross-lane reduction.
//   k_tt_select   a wave per plane: every lane keeps the first largest score of its indices (strictly greater from -1.0: a NaN is never kept), a butterfly keeps the
//                 larger of two and, of equal ones, the lower index -- what the reference's loop keeps.
// Everything that decides anything is __host__ __device__: tests/cxx/text_theta_host.hip runs it on the CPU.  fp64 throughout, one rounding per operation, no contraction.
#pragma once
#pragma clang fp contract(off)
#include "tsjacobi.h"

#define TT_T 256
#define TT_TH 5.991f               // SolveTheta's `const float th = 5.991`, compared and subtracted as a double

struct TtDev {
    int n_plane; const int32_t *off, *hyp_off, *triple; const float *host_xy, *targ_xy; const double *rho_in; double T[12], K[4];
    int32_t *sel; double *theta, *score; float *p3d; double *rho; double *hyp_score, *hyp_theta;
};

// tool::PixToCam: (p.x - cx)/fx in double, stored in a cv::Point2f
__host__ __device__ __forceinline__ float tt_pix_to_cam(float p, double c, double f) { return (float)(((double)p - c)/f); }

// cvTriangulatePoints' point of one feature (as recalled) between the cameras P1 and P2 = T (3 x 4, row-major), and what GetTextTheta / GetForTriangular make of it:
// X = p4d / p4d(3) in float, rho = 1/z.  The null vector's sign cancels: the reciprocal and the products change sign together.
__host__ __device__ inline void tt_triangulate_between(const double P1[12], const double T[12], const double K[4], const float *h, const float *t, float X[3], double &rho) {
    const double x1 = (double)tt_pix_to_cam(h[0], K[2], K[0]), y1 = (double)tt_pix_to_cam(h[1], K[3], K[1]);
    const double x2 = (double)tt_pix_to_cam(t[0], K[2], K[0]), y2 = (double)tt_pix_to_cam(t[1], K[3], K[1]);
    double G[4][4], vd[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        G[0][j] = x1*P1[8 + j] - P1[j]; G[1][j] = y1*P1[8 + j] - P1[4 + j];
        G[2][j] = x2*T[8 + j] - T[j];   G[3][j] = y2*T[8 + j] - T[4 + j]; }
    jac_null4(G, vd);
    const float v[4] = { (float)vd[0], (float)vd[1], (float)vd[2], (float)vd[3] };
    const float r = (float)(1.0/(double)v[3]);                             // Mat /= scalar: the reciprocal in double, rounded to float, a float product per entry
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = TS_FMUL(v[i], r);
    rho = 1.0/(double)X[2];
}
// ... between P1 = [I | 0] and P2 = T: GetTextTheta's
__host__ __device__ inline void tt_triangulate(const double T[12], const double K[4], const float *h, const float *t, float X[3], double &rho) {
    const double P1[12] = { 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0 };
    tt_triangulate_between(P1, T, K, h, t, X, rho);
}

// a feature's host ray (tool::GetRayRho, tracking.cc:352-354) and its target pixel, as the doubles SolveTheta reads
__host__ __device__ __forceinline__ void tt_feature(const double K[4], const float *h, const float *t, double rho, double f[5]) {
    f[0] = ((double)h[0] - K[2])/K[0]; f[1] = ((double)h[1] - K[3])/K[1]; f[2] = rho; f[3] = (double)t[0]; f[4] = (double)t[1];
}

// SolveTheta's closed form (tracking.cc:1883-1892, initializer.cc:1021-1030), operation by operation; m1, m2, m3 = (ray x, ray y, rho) of the triple
__host__ __device__ __forceinline__ void tt_solve(const double m1[3], const double m2[3], const double m3[3], double th[3]) {
    const double A = m3[1]/m3[0];
    const double B = 1.0/m3[0];
    const double C = (1.0 - m2[0]*B)/(m2[1] - m2[0]*A);
    const double D = (((A*C - B)*m1[0]) - C*m1[1]) + 1.0;
    const double rho3pie = m3[2]/m3[0];
    const double rho2pie = (m2[2] - rho3pie*m2[0])/(m2[1] - m2[0]*A);
    const double rho1pie = (m1[2] - rho3pie*m1[0]) - rho2pie*(m1[1] - A*m1[0]);
    th[2] = rho1pie/D;
    th[1] = rho2pie - C*th[2];
    th[0] = (rho3pie - A*th[1]) - B*th[2];
}

// one feature's term of SolveTheta's loop (:1896-1912): true and `term` = th - chi, or false for chi > th.  A NaN chi is not greater: its term is NaN.
__host__ __device__ __forceinline__ bool tt_term(const double T[12], const double K[4], const double th[3], double m0, double m1, double tx, double ty, double &term) {
    const double rhoPred = (m0*th[0] + m1*th[1]) + 1.0*th[2];
    const double inv = 1.0/rhoPred;
    const double P0 = ((T[0]*m0 + T[1]*m1) + T[2]*1.0)*inv + T[3];
    const double P1 = ((T[4]*m0 + T[5]*m1) + T[6]*1.0)*inv + T[7];
    const double P2 = ((T[8]*m0 + T[9]*m1) + T[10]*1.0)*inv + T[11];
    const double u = P0/P2*K[0] + K[2], v = P1/P2*K[1] + K[3];
    const double eu = tx - u, ev = ty - v;
    const double chi = eu*eu + ev*ev, lim = (double)TT_TH;
    if (chi > lim) return false;
    term = lim - chi;
    return true;
}

// a hypothesis: its score over the plane's n features (f0 .. f4: arrays of the five doubles of tt_feature) and the NEGATED theta the reference returns
__host__ __device__ inline double tt_hypothesis(const double T[12], const double K[4], int n, const double *f0, const double *f1, const double *f2, const double *f3, const double *f4,
                                                const int32_t tri[3], double out[3]) {
    const double m1[3] = { f0[tri[0]], f1[tri[0]], f2[tri[0]] }, m2[3] = { f0[tri[1]], f1[tri[1]], f2[tri[1]] }, m3[3] = { f0[tri[2]], f1[tri[2]], f2[tri[2]] };
    double th[3], score = 0.0;
    tt_solve(m1, m2, m3, th);
#pragma unroll 1
    for (int i = 0; i < n; i++) { double term;
        if (tt_term(T, K, th, f0[i], f1[i], f3[i], f4[i], term)) score += term; }
    out[0] = -th[0]; out[1] = -th[1]; out[2] = -th[2];
    return score;
}

// GetTextTheta's keep loop (:1712-1725) over the indices lane, lane + nl, ...: `BestScore < score` from -1.0
__host__ __device__ __forceinline__ void tt_scan(const double *score, int nh, int lane, int nl, double &best, int &idx) {
    best = -1.0; idx = -1;
    for (int i = lane; i < nh; i += nl) { const double s = score[i]; if (best < s) { best = s; idx = i; } }
}
// of two lanes' kept ones: the larger score, the lower index of equal scores (-1 = nothing kept counts as the highest index)
__host__ __device__ __forceinline__ bool tt_takes(double a, int ia, double b, int ib) { return b > a || (b == a && (unsigned)ib < (unsigned)ia); }

__global__ __launch_bounds__(TT_T) void k_tt_rho(TtDev D, int N) {
    const int i = blockIdx.x*TT_T + threadIdx.x;
    if (i >= N) return;
    float X[3] = { 0.f, 0.f, 0.f }; double rho;
    if (D.rho_in) rho = D.rho_in[i];
    else tt_triangulate(D.T, D.K, D.host_xy + 2*(size_t)i, D.targ_xy + 2*(size_t)i, X, rho);
    D.rho[i] = rho; D.p3d[3*(size_t)i] = X[0]; D.p3d[3*(size_t)i + 1] = X[1]; D.p3d[3*(size_t)i + 2] = X[2];
}

__global__ __launch_bounds__(TT_T) void k_tt_score(TtDev D) {
    __shared__ double s_f[5][TSORB_THETA_MAX_FEAT];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int a = D.off[p], n = D.off[p + 1] - a, h0 = D.hyp_off[p], nh = D.hyp_off[p + 1] - h0, first = blockIdx.y*TT_T;
    if (first >= nh) return;                                               // uniform over the workgroup
    const int h = first + tid;
    if (n < 3) {                                                           // nothing to solve: the plane's hypotheses report zeros
        if (h < nh) { const size_t e = (size_t)(h0 + h); D.hyp_score[e] = 0.0; D.hyp_theta[3*e] = 0.0; D.hyp_theta[3*e + 1] = 0.0; D.hyp_theta[3*e + 2] = 0.0; }
        return; }
    for (int i = tid; i < n; i += TT_T) { double f[5]; const size_t g = (size_t)(a + i);       // n <= TSORB_THETA_MAX_FEAT: checked by the call
        tt_feature(D.K, D.host_xy + 2*g, D.targ_xy + 2*g, D.rho[g], f);
        s_f[0][i] = f[0]; s_f[1][i] = f[1]; s_f[2][i] = f[2]; s_f[3][i] = f[3]; s_f[4][i] = f[4]; }
    __syncthreads();
    if (h >= nh) return;                                                   // (no barrier below)
    const size_t e = (size_t)(h0 + h);
    const int32_t tri[3] = { D.triple[3*e], D.triple[3*e + 1], D.triple[3*e + 2] };            // within [0, n): checked by the call
    double th[3];
    const double score = tt_hypothesis(D.T, D.K, n, s_f[0], s_f[1], s_f[2], s_f[3], s_f[4], tri, th);
    D.hyp_score[e] = score; D.hyp_theta[3*e] = th[0]; D.hyp_theta[3*e + 1] = th[1]; D.hyp_theta[3*e + 2] = th[2];
}

__global__ __launch_bounds__(64) void k_tt_select(TtDev D) {
    const int lane = threadIdx.x, p = blockIdx.x;
    const int n = D.off[p + 1] - D.off[p], h0 = D.hyp_off[p], nh = n < 3 ? 0 : D.hyp_off[p + 1] - h0;
    double best; int idx;
    tt_scan(D.hyp_score + h0, nh, lane, 64, best, idx);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) { const double b = __shfl_xor(best, m); const int ib = __shfl_xor(idx, m);
        if (tt_takes(best, idx, b, ib)) { best = b; idx = ib; } }
    if (lane == 0) { D.sel[p] = idx; D.score[p] = idx >= 0 ? best : 0.0; }
    if (lane < 3) D.theta[3*(size_t)p + lane] = idx >= 0 ? D.hyp_theta[3*(size_t)(h0 + idx) + lane] : 0.0;
}
