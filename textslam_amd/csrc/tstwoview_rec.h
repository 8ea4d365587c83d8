// tstwoview_rec.h -- initializer::ReconstructH / ReconstructF on the device (tsorb_match_two_view_reconstruct, include/tsorb.h; docs/twoview_reconstruct_recalled.md is
// the arithmetic).  Three launches, no workgroup waits for another:
//   k_rec_pairs   one thread per (hypothesis, match), a workgroup per (256 matches, hypothesis).  Lane 0 forms the workgroup's hypothesis (the 3 x 3 SVD by the one-sided
//                 iteration in registers, the Faugeras / DecomposeE formulas in fp64, R and t rounded to float once) and CheckRT's P2 and O2; then every lane
//                 triangulates its match: the 4 x 4 of the reference's float products, its null vector by the one-sided iteration on the four columns in fp64 --
//                 the matrix and the accumulated rotations in registers, the pair loops unrolled with constant indices, a lane turning until ITS matrix has
//                 converged -- the point rounded to float once, and CheckRT's float arithmetic on it to the bit: the exit the match took, its point and its cosine.
//   k_rec_stat    a workgroup per hypothesis: nGood from ballots over the exits, the cosine CheckRT picks (sorted[min(50, nGood - 1)]) by a radix select on the float
//                 bit patterns with a 256-bin histogram in LDS (four passes of eight bits), the parallax.
//   k_rec_keep    lane 0 of every workgroup runs the keep logic of ReconstructH / ReconstructF over the eight counts (a few comparisons: cheaper than a launch of its
//                 own), then the workgroup writes its 256 matches of the kept hypothesis' p3d / triangulated; workgroup 0 writes result, R21 and t21.
// Everything that decides anything is __host__ __device__ with the lane and the lane count as arguments: tests/cxx/two_view_reconstruct_host.hip calls it with (0, 1).
#pragma once
#pragma clang fp contract(off)
#include "tsjacobi.h"

#define REC_T 256
#define REC_NW (REC_T/64)
#define REC_COS_LOW 0.99998       // CheckRT's cosParallax < 0.99998, a double constant against the float cosine
#define REC_RATIO 1.00001         // ReconstructH's d1/d2 < 1.00001 || d2/d3 < 1.00001
#define REC_PI 3.1415926535897932384626433832795     // CV_PI
// hyp_state: the exit a match took in a hypothesis
#define REC_ST_OUT 0              // not an inlier of the model (or nothing was evaluated)
#define REC_ST_NONFINITE 1        // a coordinate of the point is not finite (or the cosine is NaN: stated difference)
#define REC_ST_DEPTH1 2
#define REC_ST_DEPTH2 3
#define REC_ST_ERR1 4
#define REC_ST_ERR2 5
#define REC_ST_GOOD 6             // counted in nGood, cosine at or above 0.99998: not triangulated
#define REC_ST_TRI 7              // counted and triangulated
// result[5]
#define REC_EXIT_SV 1             // H only: d1/d2 or d2/d3 below 1.00001
#define REC_EXIT_FEW 2            // not enough good points
#define REC_EXIT_TIE 4            // no clear winner
#define REC_EXIT_PARALLAX 8

struct RecHyp { float R[9], t[3]; };               // a motion hypothesis, rounded to float once
struct RecCam { float P2[12], O2[3]; };            // CheckRT's P2 = K [R | t] and O2 = -R^T t

struct RecDev {
    int n, model, n_inl, min_tri; const float *xy1, *xy2; const uint8_t *inl; float M[9], K[4], sigma, min_par;
    int32_t *result; float *R21, *t21, *p3d; uint8_t *tri; int32_t *hyp_good; float *hyp_cos, *hyp_par, *hyp_pose; uint8_t *hyp_state; float *hyp_p3d;
    float *cosall; int32_t *sv_exit;               // device only: every pair's cosine [8][n]; ReconstructH's singular-value exit was taken
};

template <int a, int b>
__host__ __device__ __forceinline__ void rec_order3(double G[3][3], double Q[3][3], double d[3]) {       // column a before column b when it is at least as long
    if (d[a] < d[b]) { double x = d[a]; d[a] = d[b]; d[b] = x;
#pragma unroll
        for (int i = 0; i < 3; i++) { x = G[i][a]; G[i][a] = G[i][b]; G[i][b] = x; x = Q[i][a]; Q[i][a] = Q[i][b]; Q[i][b] = x; } }
}

// A = U diag(d) V^T, d descending: G = A Q with orthogonal columns (tsjacobi.h's one-sided iteration), d_j = |G_j|, v_j = Q_j; u_j = G_j / d_j is left to the caller
__host__ __device__ inline void rec_svd3(const double A[9], double G[3][3], double Q[3][3], double d[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = A[3*i + j];
    jac_orthogonalize(G, Q, JAC_ORTHO, JAC_TINY);
#pragma unroll
    for (int j = 0; j < 3; j++) d[j] = sqrt(jac_length2(G, j));
    rec_order3<0, 1>(G, Q, d); rec_order3<1, 2>(G, Q, d); rec_order3<0, 1>(G, Q, d);
}

__host__ __device__ __forceinline__ void rec_cross(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1]*b[2] - a[2]*b[1]; c[1] = a[2]*b[0] - a[0]*b[2]; c[2] = a[0]*b[1] - a[1]*b[0];
}
__host__ __device__ __forceinline__ double rec_det3(const double a[3], const double b[3], const double c[3]) {      // of the matrix with columns a, b, c
    double x[3]; rec_cross(b, c, x); return (a[0]*x[0] + a[1]*x[1]) + a[2]*x[2];
}

// R = sg (w0 v0^T + w1 v1^T + w2 v2^T) and t = tt / |tt|, each entry rounded to float once
__host__ __device__ __forceinline__ void rec_round(double sg, const double w0[3], const double w1[3], const double w2[3], const double v0[3], const double v1[3], const double v2[3],
                                                   const double tt[3], RecHyp &o) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) o.R[3*i + j] = (float)(sg*((w0[i]*v0[j] + w1[i]*v1[j]) + w2[i]*v2[j]));
    const double nn = sqrt((tt[0]*tt[0] + tt[1]*tt[1]) + tt[2]*tt[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = (float)(tt[i]/nn);
}

// ReconstructH's hypothesis h (0 .. 7) from the float H21 and K (:648-752).  true: the singular-value exit (:661), nothing formed
__host__ __device__ inline bool rec_hyp_h(const float H[9], const float K[4], int h, RecHyp &o) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    double A[9], G[3][3], Q[3][3], d[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {                                          // A = K^-1 (H K)
        const double h0 = c == 0 ? (double)H[0]*fx : c == 1 ? (double)H[1]*fy : ((double)H[0]*cx + (double)H[1]*cy) + (double)H[2];
        const double h1 = c == 0 ? (double)H[3]*fx : c == 1 ? (double)H[4]*fy : ((double)H[3]*cx + (double)H[4]*cy) + (double)H[5];
        const double h2 = c == 0 ? (double)H[6]*fx : c == 1 ? (double)H[7]*fy : ((double)H[6]*cx + (double)H[7]*cy) + (double)H[8];
        A[c] = (h0 - cx*h2)/fx; A[3 + c] = (h1 - cy*h2)/fy; A[6 + c] = h2; }
    rec_svd3(A, G, Q, d);
    const float d1f = (float)d[0], d2f = (float)d[1], d3f = (float)d[2];
    if ((double)TS_FDIV(d1f, d2f) < REC_RATIO || (double)TS_FDIV(d2f, d3f) < REC_RATIO) return true;
    double u[3][3], v[3][3];                                               // u[j], v[j]: the j-th left / right singular vector
#pragma unroll
    for (int j = 0; j < 3; j++) { const bool neg = j != 1 && jac_negative3(Q[0][j], Q[1][j], Q[2][j]);
#pragma unroll
        for (int i = 0; i < 3; i++) { v[j][i] = neg ? -Q[i][j] : Q[i][j]; u[j][i] = (neg ? -G[i][j] : G[i][j])/d[j]; } }
    const double sg = rec_det3(u[0], u[1], u[2])*rec_det3(v[0], v[1], v[2]) < 0.0 ? -1.0 : 1.0;
    const double d1 = d[0], d2 = d[1], d3 = d[2], q12 = d1*d1 - d2*d2, q23 = d2*d2 - d3*d3, q13 = d1*d1 - d3*d3;
    const int i = h & 3; const double e1 = i < 2 ? 1.0 : -1.0, e3 = (i & 1) ? -1.0 : 1.0;
    const double x1 = e1*sqrt(q12/q13), x3 = e3*sqrt(q23/q13);
    double w0[3], w1[3], w2[3], tt[3];
    if (h < 4) {                                                           // d' = d2
        const double st = e1*e3*(sqrt(q12*q23)/((d1 + d3)*d2)), ct = (d2*d2 + d1*d3)/((d1 + d3)*d2);
#pragma unroll
        for (int k = 0; k < 3; k++) { w0[k] = ct*u[0][k] + st*u[2][k]; w1[k] = u[1][k]; w2[k] = ct*u[2][k] - st*u[0][k];
            tt[k] = (x1*(d1 - d3))*u[0][k] + (-x3*(d1 - d3))*u[2][k]; }
    } else {                                                               // d' = -d2
        const double sp = e1*e3*(sqrt(q12*q23)/((d1 - d3)*d2)), cp = (d1*d3 - d2*d2)/((d1 - d3)*d2);
#pragma unroll
        for (int k = 0; k < 3; k++) { w0[k] = cp*u[0][k] + sp*u[2][k]; w1[k] = -u[1][k]; w2[k] = sp*u[0][k] - cp*u[2][k];
            tt[k] = (x1*(d1 + d3))*u[0][k] + (x3*(d1 + d3))*u[2][k]; }
    }
    rec_round(sg, w0, w1, w2, v[0], v[1], v[2], tt, o);
    return false;
}

// ReconstructF's hypothesis h (0 .. 3): (R1, t), (R2, t), (R1, -t), (R2, -t) from the float F21 and K (:540-548, DecomposeE :979-999)
__host__ __device__ inline void rec_hyp_f(const float F[9], const float K[4], int h, RecHyp &o) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    double E[9], G[3][3], Q[3][3], d[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {                                          // E = K^T (F K)
        const double f0 = c == 0 ? (double)F[0]*fx : c == 1 ? (double)F[1]*fy : ((double)F[0]*cx + (double)F[1]*cy) + (double)F[2];
        const double f1 = c == 0 ? (double)F[3]*fx : c == 1 ? (double)F[4]*fy : ((double)F[3]*cx + (double)F[4]*cy) + (double)F[5];
        const double f2 = c == 0 ? (double)F[6]*fx : c == 1 ? (double)F[7]*fy : ((double)F[6]*cx + (double)F[7]*cy) + (double)F[8];
        E[c] = fx*f0; E[3 + c] = fy*f1; E[6 + c] = (cx*f0 + cy*f1) + f2; }
    rec_svd3(E, G, Q, d);
    double u[3][3], v[3][3];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) { v[j][i] = Q[i][j]; u[j][i] = G[i][j]/d[j]; }
    rec_cross(u[0], u[1], u[2]); rec_cross(v[0], v[1], v[2]);              // det U = det V = +1: both products below are rotations
    // U W V^T = u2 v1^T - u1 v2^T + u3 v3^T and U W^T V^T = -u2 v1^T + u1 v2^T + u3 v3^T; their traces decide which is R1
    double tra = 0.0, trb = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) { const double a = u[1][k]*v[0][k] - u[0][k]*v[1][k], b = u[2][k]*v[2][k]; tra += a + b; trb += b - a; }
    const bool first = ((h & 1) == 0) == (tra >= trb);                     // this hypothesis takes U W V^T
    const bool neg = jac_negative3(u[2][0], u[2][1], u[2][2]) != ((h & 2) != 0);
    double w0[3], w1[3], tt[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { w0[k] = first ? u[1][k] : -u[1][k]; w1[k] = first ? -u[0][k] : u[0][k]; tt[k] = neg ? -u[2][k] : u[2][k]; }
    rec_round(1.0, w0, w1, u[2], v[0], v[1], v[2], tt, o);
}

// CheckRT's P2 = K [R | t] and O2 = -R^T t (:891-896): cv::gemm on CV_32F, double accumulation and one float rounding per entry (as recalled)
__host__ __device__ inline void rec_camera(const RecHyp &hp, const float K[4], RecCam &cam) {
#pragma unroll
    for (int j = 0; j < 4; j++) { const double r0 = j < 3 ? hp.R[j] : hp.t[0], r1 = j < 3 ? hp.R[3 + j] : hp.t[1], r2 = j < 3 ? hp.R[6 + j] : hp.t[2];
        cam.P2[j] = (float)((double)K[0]*r0 + (double)K[2]*r2); cam.P2[4 + j] = (float)((double)K[1]*r1 + (double)K[3]*r2); cam.P2[8 + j] = (float)r2; }
#pragma unroll
    for (int i = 0; i < 3; i++) cam.O2[i] = (float)(-(((double)hp.R[i]*(double)hp.t[0] + (double)hp.R[3 + i]*(double)hp.t[1]) + (double)hp.R[6 + i]*(double)hp.t[2]));
}

__host__ __device__ __forceinline__ float rec_th2(float sigma) { return (float)(4.0*(double)TS_FMUL(sigma, sigma)); }

// initializer::Triangulate (:804-817): the rows are the reference's float products and differences; from that float matrix on fp64 -- the right singular vector of
// the smallest singular value (the first of equal ones) -- and X = v[0 .. 2] / v[3] rounded to float once
__host__ __device__ inline void rec_triangulate(const RecCam &cam, const float K[4], float x1, float y1, float x2, float y2, float X[3]) {
    const float P1[12] = { K[0], 0.f, K[2], 0.f, 0.f, K[1], K[3], 0.f, 0.f, 0.f, 1.f, 0.f };
    double G[4][4], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        G[0][j] = (double)TS_FSUB(TS_FMUL(x1, P1[8 + j]), P1[j]); G[1][j] = (double)TS_FSUB(TS_FMUL(y1, P1[8 + j]), P1[4 + j]);
        G[2][j] = (double)TS_FSUB(TS_FMUL(x2, cam.P2[8 + j]), cam.P2[j]); G[3][j] = (double)TS_FSUB(TS_FMUL(y2, cam.P2[8 + j]), cam.P2[4 + j]); }
    jac_null4(G, v);
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = (float)(v[i]/v[3]);
}

__host__ __device__ __forceinline__ float rec_norm3(float x, float y, float z) {       // cv::norm (NORM_L2) of a CV_32F 3-vector: double accumulation (as recalled)
    return (float)sqrt(((double)x*(double)x + (double)y*(double)y) + (double)z*(double)z);
}
__host__ __device__ __forceinline__ float rec_project(float f, float x, float invz, float c) { return TS_FADD(TS_FMUL(TS_FMUL(f, x), invz), c); }
__host__ __device__ __forceinline__ float rec_err(float ax, float px, float ay, float py) {
    const float dx = TS_FSUB(ax, px), dy = TS_FSUB(ay, py); return TS_FADD(TS_FMUL(dx, dx), TS_FMUL(dy, dy));
}

// CheckRT's loop body after Triangulate (:911-963) on the FLOAT point X: the exit it takes and the cosine, the reference's arithmetic to the bit
__host__ __device__ inline int rec_check(const RecHyp &hp, const RecCam &cam, const float K[4], float th2, float x1, float y1, float x2, float y2, const float X[3], float &cosv) {
    cosv = 0.f;
    if (!__builtin_isfinite(X[0]) || !__builtin_isfinite(X[1]) || !__builtin_isfinite(X[2])) return REC_ST_NONFINITE;
    const float a0 = TS_FSUB(X[0], 0.f), a1 = TS_FSUB(X[1], 0.f), a2 = TS_FSUB(X[2], 0.f);                               // normal1 = p3dC1 - O1
    const float b0 = TS_FSUB(X[0], cam.O2[0]), b1 = TS_FSUB(X[1], cam.O2[1]), b2 = TS_FSUB(X[2], cam.O2[2]);             // normal2 = p3dC1 - O2
    const float dist1 = rec_norm3(a0, a1, a2), dist2 = rec_norm3(b0, b1, b2);
    const double dot = ((double)a0*(double)b0 + (double)a1*(double)b1) + (double)a2*(double)b2;                       // Mat::dot: double accumulation (as recalled)
    const float c = (float)(dot/(double)TS_FMUL(dist1, dist2));
    if (c != c) return REC_ST_NONFINITE;                                   // stated difference: the reference would hand a NaN to std::sort
    cosv = c;
    const bool low = (double)c < REC_COS_LOW;
    if (X[2] <= 0.f && low) return REC_ST_DEPTH1;
    float p2[3];
#pragma unroll
    for (int i = 0; i < 3; i++)                                            // R * p3dC1 + t: one gemm, double accumulation, one rounding (as recalled)
        p2[i] = (float)(((((double)hp.R[3*i]*(double)X[0] + (double)hp.R[3*i + 1]*(double)X[1]) + (double)hp.R[3*i + 2]*(double)X[2])) + (double)hp.t[i]);
    if (p2[2] <= 0.f && low) return REC_ST_DEPTH2;
    const float iz1 = (float)(1.0/(double)X[2]);
    if (rec_err(rec_project(K[0], X[0], iz1, K[2]), x1, rec_project(K[1], X[1], iz1, K[3]), y1) > th2) return REC_ST_ERR1;
    const float iz2 = (float)(1.0/(double)p2[2]);
    if (rec_err(rec_project(K[0], p2[0], iz2, K[2]), x2, rec_project(K[1], p2[1], iz2, K[3]), y2) > th2) return REC_ST_ERR2;
    return low ? REC_ST_TRI : REC_ST_GOOD;
}

// a float's bit pattern as an unsigned key in the order of the floats (-0 before +0; no NaN gets here)
__host__ __device__ __forceinline__ uint32_t rec_key(float c) {
    union { float f; uint32_t u; } x; x.f = c;
    return (x.u & 0x80000000u) ? ~x.u : (x.u | 0x80000000u);
}
__host__ __device__ __forceinline__ float rec_unkey(uint32_t k) {
    union { float f; uint32_t u; } x; x.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return x.f;
}

// the key of rank k (0-based, ascending) among the counted matches' cosines: four passes of eight bits over a 256-bin histogram (lanes; hist is LDS on the device)
__host__ __device__ inline uint32_t rec_select(const uint8_t *state, const float *cosv, int n, int k, uint32_t *hist, int lane, int nl) {
    uint32_t prefix = 0; int rem = k;
#pragma unroll 1
    for (int pass = 0; pass < 4; pass++) { const int shift = 24 - 8*pass;
        for (int b = lane; b < 256; b += nl) hist[b] = 0;
        TS_BARRIER();
        for (int i = lane; i < n; i += nl) if (state[i] >= REC_ST_GOOD) { const uint32_t key = rec_key(cosv[i]);
            if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) TS_COUNT(hist[(key >> shift) & 255u]); }
        TS_BARRIER();
        int acc = 0, bsel = 255, before = 0; bool found = false;           // every lane reads all 256 bins (independent broadcast reads) and arrives at the same bin
        for (int b = 0; b < 256; b++) { const int cnt = (int)hist[b];
            if (!found && rem < acc + cnt) { found = true; bsel = b; before = acc; }
            acc += cnt; }
        rem -= before; prefix |= (uint32_t)bsel << shift;
        TS_BARRIER();
    }
    return prefix;
}

// CheckRT's parallax (:971): acos of the float, * 180 in float, / CV_PI in double, stored in a float
__host__ __device__ __forceinline__ float rec_parallax(float c) { return (float)((double)TS_FMUL(acosf(c), 180.f)/REC_PI); }

// the keep logic of ReconstructH (:755-801) or ReconstructF (:560-633) over the hypotheses' counts and parallaxes, comparison for comparison.
// res = ok, sel (-1 unless ok), N, best nGood, second best nGood (H) / nsimilar (F), exit bits
__host__ __device__ inline void rec_keep(int model, bool sv_exit, const int32_t *good, const float *par, int N, int min_tri, float min_par, int32_t res[6]) {
    res[0] = 0; res[1] = -1; res[2] = N; res[3] = 0; res[4] = 0; res[5] = 0;
    if (model == 0) {
        if (sv_exit) { res[5] = REC_EXIT_SV; return; }
        int best = 0, second = 0, idx = -1; float bpar = -1.f;
#pragma unroll
        for (int i = 0; i < 8; i++) { const int g = good[i];
            if (g > best) { second = best; best = g; idx = i; bpar = par[i]; }
            else if (g > second) second = g; }
        const bool c0 = (double)second < 0.75*(double)best, c1 = bpar >= min_par, c2 = best > min_tri, c3 = (double)best > 0.9*(double)N;
        res[3] = best; res[4] = second;
        res[5] = (c0 ? 0 : REC_EXIT_TIE) | (c1 ? 0 : REC_EXIT_PARALLAX) | (c2 && c3 ? 0 : REC_EXIT_FEW);
        if (res[5] == 0) { res[0] = 1; res[1] = idx; }
    } else {
        const int g0 = good[0], g1 = good[1], g2 = good[2], g3 = good[3];
        const int m23 = g2 > g3 ? g2 : g3, m123 = g1 > m23 ? g1 : m23, mx = g0 > m123 ? g0 : m123;
        const int few = (int)(0.9*(double)N), nmin = few > min_tri ? few : min_tri;
        const double lim = 0.7*(double)mx;
        const int nsim = ((double)g0 > lim ? 1 : 0) + ((double)g1 > lim ? 1 : 0) + ((double)g2 > lim ? 1 : 0) + ((double)g3 > lim ? 1 : 0);
        res[3] = mx; res[4] = nsim;
        res[5] = (mx < nmin ? REC_EXIT_FEW : 0) | (nsim > 1 ? REC_EXIT_TIE : 0);
        if (res[5]) return;
        const int idx = mx == g0 ? 0 : mx == g1 ? 1 : mx == g2 ? 2 : 3;
        const float p = idx == 0 ? par[0] : idx == 1 ? par[1] : idx == 2 ? par[2] : par[3];
        if (p > min_par) { res[0] = 1; res[1] = idx; } else res[5] = REC_EXIT_PARALLAX;
    }
}

// hypothesis h of the model and its camera; true: ReconstructH's singular-value exit
__host__ __device__ inline bool rec_form(int model, const float M[9], const float K[4], int h, RecHyp &hp, RecCam &cam) {
    if (model == 0) { if (rec_hyp_h(M, K, h, hp)) return true; } else rec_hyp_f(M, K, h, hp);
    rec_camera(hp, K, cam);
    return false;
}

// one (hypothesis, match): the exit, the float point (zeros for a match that is not evaluated) and the cosine
__host__ __device__ inline int rec_pair(const RecHyp &hp, const RecCam &cam, const float K[4], float th2, bool inlier, const float *p1, const float *p2, float X[3], float &cosv) {
    X[0] = 0.f; X[1] = 0.f; X[2] = 0.f; cosv = 0.f;
    if (!inlier) return REC_ST_OUT;
    rec_triangulate(cam, K, p1[0], p1[1], p2[0], p2[1], X);
    return rec_check(hp, cam, K, th2, p1[0], p1[1], p2[0], p2[1], X, cosv);
}

__global__ __launch_bounds__(REC_T) void k_rec_pairs(RecDev D) {
    __shared__ RecHyp s_hp; __shared__ RecCam s_cam; __shared__ int s_exit;
    const int tid = threadIdx.x, h = blockIdx.y, i = blockIdx.x*REC_T + tid;
    if (tid == 0) s_exit = rec_form(D.model, D.M, D.K, h, s_hp, s_cam) ? 1 : 0;
    __syncthreads();
    const bool ex = s_exit != 0;
    if (blockIdx.x == 0) {
        if (tid < 12) { D.hyp_pose[12*h + tid] = ex ? 0.f : (tid%4 < 3 ? s_hp.R[3*(tid/4) + tid%4] : s_hp.t[tid/4]);
            if (D.model == 1) D.hyp_pose[12*(h + 4) + tid] = 0.f; }
        if (tid == 0 && h == 0) D.sv_exit[0] = s_exit;
    }
    if (i >= D.n) return;                                                  // (no barrier below)
    float X[3] = { 0.f, 0.f, 0.f }, cosv = 0.f; int st = REC_ST_OUT;
    if (!ex) st = rec_pair(s_hp, s_cam, D.K, rec_th2(D.sigma), D.inl[i] != 0, D.xy1 + 2*(size_t)i, D.xy2 + 2*(size_t)i, X, cosv);
    const size_t e = (size_t)h*D.n + i;
    D.hyp_state[e] = (uint8_t)st; D.cosall[e] = cosv; D.hyp_p3d[3*e] = X[0]; D.hyp_p3d[3*e + 1] = X[1]; D.hyp_p3d[3*e + 2] = X[2];
    if (D.model == 1) { const size_t z = e + 4*(size_t)D.n;                 // F has four hypotheses: the other four report nothing
        D.hyp_state[z] = REC_ST_OUT; D.hyp_p3d[3*z] = 0.f; D.hyp_p3d[3*z + 1] = 0.f; D.hyp_p3d[3*z + 2] = 0.f; }
}

__global__ __launch_bounds__(REC_T) void k_rec_stat(RecDev D) {
    __shared__ uint32_t s_hist[256]; __shared__ int s_cnt[REC_NW];
    const int tid = threadIdx.x, h = blockIdx.x, nh = D.model == 0 ? 8 : 4;
    if (h >= nh || D.sv_exit[0] != 0) {                                     // uniform over the workgroup
        if (tid == 0) { D.hyp_good[h] = 0; D.hyp_cos[h] = 0.f; D.hyp_par[h] = 0.f; }
        return; }
    const uint8_t *state = D.hyp_state + (size_t)h*D.n; const float *cosv = D.cosall + (size_t)h*D.n;
    int cnt = 0;
    for (int base = 0; base < D.n; base += REC_T) { const int i = base + tid;                                       // the same trip count for every lane
        cnt += __popcll(__ballot(i < D.n && state[i] >= REC_ST_GOOD)); }
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    int good = 0;
#pragma unroll
    for (int w = 0; w < REC_NW; w++) good += s_cnt[w];
    float c = 0.f, par = 0.f;
    if (good > 0) {                                                        // uniform over the workgroup
        c = rec_unkey(rec_select(state, cosv, D.n, good - 1 < 50 ? good - 1 : 50, s_hist, tid, REC_T));
        par = rec_parallax(c); }
    if (tid == 0) { D.hyp_good[h] = good; D.hyp_cos[h] = c; D.hyp_par[h] = par; }
}

__global__ __launch_bounds__(REC_T) void k_rec_keep(RecDev D) {
    __shared__ int32_t s_res[6];
    const int tid = threadIdx.x, i = blockIdx.x*REC_T + tid;
    if (tid == 0) rec_keep(D.model, D.sv_exit[0] != 0, D.hyp_good, D.hyp_par, D.n_inl, D.min_tri, D.min_par, s_res);
    __syncthreads();
    const int sel = s_res[1];
    if (blockIdx.x == 0) {
        if (tid < 6) D.result[tid] = s_res[tid];
        if (tid < 9) D.R21[tid] = sel >= 0 ? D.hyp_pose[12*sel + 4*(tid/3) + tid%3] : 0.f;
        if (tid < 3) D.t21[tid] = sel >= 0 ? D.hyp_pose[12*sel + 4*tid + 3] : 0.f;
    }
    if (i >= D.n) return;
    const size_t e = (size_t)(sel >= 0 ? sel : 0)*D.n + i;
    const int st = sel >= 0 ? D.hyp_state[e] : REC_ST_OUT; const bool good = st >= REC_ST_GOOD;
    D.p3d[3*(size_t)i] = good ? D.hyp_p3d[3*e] : 0.f; D.p3d[3*(size_t)i + 1] = good ? D.hyp_p3d[3*e + 1] : 0.f; D.p3d[3*(size_t)i + 2] = good ? D.hyp_p3d[3*e + 2] : 0.f;
    D.tri[i] = st == REC_ST_TRI ? 1 : 0;
}
