// tsloop_ransac.h -- k_sim3_batch: every loop candidate's Sim3Solver RANSAC and OptimizeSim3 in one launch (tsloop_sim3_batch, include/tsloop.h).
// Included by tsloop.hip after sim3_lm_body.  One 256-thread workgroup per candidate with at least one hypothesis; no workgroup waits for another.
//   (a) lane h < H of wave 0 forms hypothesis h: Horn's closed form from three matches (src/Sim3Solver.cc:124-193), the eigenvector by a cyclic Jacobi
//       iteration on the symmetric 4 x 4 in fp64 (docs/sim3solver_recalled.md), T12 | T21 | (q t s) into LDS
//   (b) every thread strides over the matches, its match in registers, and tests it against every hypothesis (CheckInliers / Project, :195-241);
//       the per-hypothesis counts are integer sums -- popcount of a wave's ballot, then the four waves through LDS: exact, order-free
//   (c) thread 0 runs iterate()'s selection loop (:96-104, :116) and writes the candidate's scalars
//   (d) the selected hypothesis' mask by evaluating that one hypothesis again: the same arithmetic, the same decisions, no n x H mask
//   (e) the LM of tsloop_optimize_sim3 (sim3_lm_body) on the candidate's slice, from the selection
// Every loop is bounded by H <= TSLOOP_RANSAC_MAX_HYP, the candidate's match count, JACOBI_SWEEPS or max_it.
#pragma once
#include "tsjacobi.h"

#define JACOBI_SWEEPS 24          // a 4 x 4 converges quadratically: 6-8 sweeps reach an exactly diagonal matrix; the bound only has to be finite
#define HYP_STRIDE 32             // doubles per hypothesis in LDS: T12 (3 x 4) | T21 (3 x 4) | q t s

struct Sim3BatchDev {
    const int32_t *cand;          // [grid]: the candidates that have hypotheses
    const int32_t *off, *hyp_off, *triple;
    const double *P1, *P2, *pred1, *pred2; const float *uv1, *uv2; const double *K2;
    double K1[4], K[4]; double max_err2; int32_t min_inliers, optimise;
    int32_t *ok, *sel, *ninl, *hyp_count; double *sim_ransac, *sim, *hyp_sim; tsloop_report *rep; uint8_t *inlier;
};

// (the per-hypothesis and per-match arithmetic is __host__ __device__: a host program can call exactly what the kernel runs)
// Horn 1987 from three matches a1[i] <-> a2[i] (points as the columns of the reference's Mat33): out = T12 (3 x 4, row-major) | T21 | qw qx qy qz t s
__host__ __device__ __forceinline__ void horn_sim3(const double a1[3][3], const double a2[3][3], double *out) {
    double O1[3], O2[3], r1[3][3], r2[3][3];                            // r*[point][axis]
#pragma unroll
    for (int a = 0; a < 3; a++) { O1[a] = ((a1[0][a] + a1[1][a]) + a1[2][a])/3.0; O2[a] = ((a2[0][a] + a2[1][a]) + a2[2][a])/3.0; }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int a = 0; a < 3; a++) { r1[i][a] = a1[i][a] - O1[a]; r2[i][a] = a2[i][a] - O2[a]; }
    double M[3][3];                                                     // M = Pr2 Pr1^T
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) M[a][b] = (r2[0][a]*r1[0][b] + r2[1][a]*r1[1][b]) + r2[2][a]*r1[2][b];
    double A[4][4], V[4][4];
    A[0][0] = M[0][0] + M[1][1] + M[2][2]; A[0][1] = M[1][2] - M[2][1]; A[0][2] = M[2][0] - M[0][2]; A[0][3] = M[0][1] - M[1][0];
    A[1][1] = M[0][0] - M[1][1] - M[2][2]; A[1][2] = M[0][1] + M[1][0]; A[1][3] = M[2][0] + M[0][2];
    A[2][2] = -M[0][0] + M[1][1] - M[2][2]; A[2][3] = M[1][2] + M[2][1];
    A[3][3] = -M[0][0] - M[1][1] + M[2][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { if (j < i) A[i][j] = A[j][i]; V[i][j] = (i == j) ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
        const double offd = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]);
        if (!(offd > 0.0)) break;                                       // diagonal (or NaN: nothing to gain)
        jac_sym_rotate<4, 0, 1>(A, V); jac_sym_rotate<4, 0, 2>(A, V); jac_sym_rotate<4, 0, 3>(A, V);
        jac_sym_rotate<4, 1, 2>(A, V); jac_sym_rotate<4, 1, 3>(A, V); jac_sym_rotate<4, 2, 3>(A, V);
    }
    double q[4] = { V[0][0], V[1][0], V[2][0], V[3][0] }, best = A[0][0];          // the first maximum, as maxCoeff
#pragma unroll
    for (int k = 1; k < 4; k++) if (A[k][k] > best) { best = A[k][k]; q[0] = V[0][k]; q[1] = V[1][k]; q[2] = V[2][k]; q[3] = V[3][k]; }
    {   const double n = sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]), sg = q[0] < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = sg*q[k]/n; }
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[9] = { 1.0 - 2.0*(y*y + z*z), 2.0*(x*y - w*z), 2.0*(x*z + w*y), 2.0*(x*y + w*z), 1.0 - 2.0*(x*x + z*z), 2.0*(y*z - w*x),
                          2.0*(x*z - w*y), 2.0*(y*z + w*x), 1.0 - 2.0*(x*x + y*y) };
    double nom = 0.0, den = 0.0;                                        // s = sum(Pr1 o R Pr2) / sum((R Pr2)^2)
#pragma unroll
    for (int i = 0; i < 3; i++) { double p3[3];
#pragma unroll
        for (int a = 0; a < 3; a++) p3[a] = R[3*a]*r2[i][0] + R[3*a + 1]*r2[i][1] + R[3*a + 2]*r2[i][2];
#pragma unroll
        for (int a = 0; a < 3; a++) { nom += r1[i][a]*p3[a]; den += p3[a]*p3[a]; } }
    const double s = nom/den, is = 1.0/s;
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; a++) t[a] = O1[a] - s*(R[3*a]*O2[0] + R[3*a + 1]*O2[1] + R[3*a + 2]*O2[2]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) { out[4*r + c] = s*R[3*r + c]; out[12 + 4*r + c] = is*R[3*c + r]; }
        out[4*r + 3] = t[r];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) out[12 + 4*r + 3] = -((out[12 + 4*r]*t[0] + out[12 + 4*r + 1]*t[1]) + out[12 + 4*r + 2]*t[2]);
#pragma unroll
    for (int k = 0; k < 4; k++) out[24 + k] = q[k];
    out[28] = t[0]; out[29] = t[1]; out[30] = t[2]; out[31] = s;
}

// squared pixel distance between pred and K (T P): the product with the 3 x 3 K, then the division (Project, :223-241); double, rounded to float
__host__ __device__ __forceinline__ float ransac_err(const double *T, const double K[4], const double P[3], const double pred[2]) {
    const double X = ((T[0]*P[0] + T[1]*P[1]) + T[2]*P[2]) + T[3], Y = ((T[4]*P[0] + T[5]*P[1]) + T[6]*P[2]) + T[7], Z = ((T[8]*P[0] + T[9]*P[1]) + T[10]*P[2]) + T[11];
    const double du = pred[0] - (K[0]*X + K[2]*Z)/Z, dv = pred[1] - (K[1]*Y + K[3]*Z)/Z;
    return (float)(du*du + dv*dv);
}
// CheckInliers, :205-220: both errors below the double threshold (a NaN compares false)
__host__ __device__ __forceinline__ bool ransac_inlier(const double *hyp, const double K1[4], const double K2[4], const double P1[3], const double P2[3],
                                              const double pr1[2], const double pr2[2], double max_err2) {
    const float e1 = ransac_err(hyp, K1, P2, pr1), e2 = ransac_err(hyp + 12, K2, P1, pr2);
    return (double)e1 < max_err2 && (double)e2 < max_err2;
}

__global__ __launch_bounds__(SIM_T) void k_sim3_batch(Sim3BatchDev B, tsloop_options o) {
    __shared__ double lds[SIM_LDS_DOUBLES];
    __shared__ double s_tot[40];
    __shared__ double s_hyp[TSLOOP_RANSAC_MAX_HYP*HYP_STRIDE];
    __shared__ int s_cnt[SIM_NW][TSLOOP_RANSAC_MAX_HYP];
    __shared__ int s_pick[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = B.cand[blockIdx.x], m0 = B.off[k], n = B.off[k + 1] - m0, h0 = B.hyp_off[k], H = B.hyp_off[k + 1] - h0;     // 1 <= H <= 64 (host)
    const double *P1 = B.P1 + 3*(size_t)m0, *P2 = B.P2 + 3*(size_t)m0, *pr1 = B.pred1 + 2*(size_t)m0, *pr2 = B.pred2 + 2*(size_t)m0;
    const double K2[4] = { B.K2[4*k], B.K2[4*k + 1], B.K2[4*k + 2], B.K2[4*k + 3] };
    // (a)
    if (tid < H) {
        double a1[3][3], a2[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++) { const int idx = B.triple[3*(h0 + tid) + i];                  // 0 <= idx < n (host)
#pragma unroll
            for (int a = 0; a < 3; a++) { a1[i][a] = P1[3*idx + a]; a2[i][a] = P2[3*idx + a]; } }
        double out[HYP_STRIDE];
        horn_sim3(a1, a2, out);
#pragma unroll
        for (int j = 0; j < HYP_STRIDE; j++) s_hyp[tid*HYP_STRIDE + j] = out[j];
#pragma unroll
        for (int j = 0; j < 8; j++) B.hyp_sim[8*(size_t)(h0 + tid) + j] = out[24 + j];
    }
    if (lane == 0) for (int h = 0; h < H; h++) s_cnt[wave][h] = 0;
    __syncthreads();
    // (b): the trip count is the same for every thread, so that a wave's ballot is whole
#pragma unroll 1
    for (int base = 0; base < n; base += SIM_T) {
        const int i = base + tid; const bool have = i < n; const int j = have ? i : 0;
        const double p1[3] = { P1[3*j], P1[3*j + 1], P1[3*j + 2] }, p2[3] = { P2[3*j], P2[3*j + 1], P2[3*j + 2] };
        const double q1[2] = { pr1[2*j], pr1[2*j + 1] }, q2[2] = { pr2[2*j], pr2[2*j + 1] };
#pragma unroll 1
        for (int h = 0; h < H; h++) {
            const bool in = have && ransac_inlier(s_hyp + h*HYP_STRIDE, B.K1, K2, p1, p2, q1, q2, B.max_err2);
            const unsigned long long b = __ballot(in);
            if (lane == 0) s_cnt[wave][h] += __popcll(b);
        }
    }
    __syncthreads();
    // (c)
    if (tid == 0) {
        int best = 0, sel = -1;
        for (int h = 0; h < H; h++) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < SIM_NW; w++) c += s_cnt[w][h];
            B.hyp_count[h0 + h] = c;
            if (c >= best) { best = c; sel = h; }                       // `>=`: the later of equal counts wins, :96
        }
        const int ok = best > B.min_inliers ? 1 : 0;                    // strict, :116
        s_pick[0] = sel; s_pick[1] = ok;
        B.sel[k] = sel; B.ok[k] = ok; B.ninl[k] = best;
        for (int j = 0; j < 8; j++) { const double v = s_hyp[sel*HYP_STRIDE + 24 + j]; B.sim_ransac[8*(size_t)k + j] = v; if (ok && B.optimise) B.sim[8*(size_t)k + j] = v; }
    }
    __syncthreads();
    // (d)
    const int sel = s_pick[0]; const bool ok = s_pick[1] != 0;
    uint8_t *inl = B.inlier + m0;
    for (int i = tid; i < n; i += SIM_T) {
        const double p1[3] = { P1[3*i], P1[3*i + 1], P1[3*i + 2] }, p2[3] = { P2[3*i], P2[3*i + 1], P2[3*i + 2] };
        const double q1[2] = { pr1[2*i], pr1[2*i + 1] }, q2[2] = { pr2[2*i], pr2[2*i + 1] };
        inl[i] = (ok && ransac_inlier(s_hyp + sel*HYP_STRIDE, B.K1, K2, p1, p2, q1, q2, B.max_err2)) ? 1 : 0;
    }
    if (!ok || !B.optimise) return;                                     // (uniform over the workgroup)
    __syncthreads();                                                    // the mask and sim[k] are written: the LM reads both
    // (e)
    Sim3Dev P; P.n = n; P.P1 = P1; P.P2 = P2; P.uv1 = B.uv1 + 2*(size_t)m0; P.uv2 = B.uv2 + 2*(size_t)m0; P.inlier = inl;
#pragma unroll
    for (int j = 0; j < 4; j++) P.K[j] = B.K[j];
    P.sim = B.sim + 8*(size_t)k; P.rep = B.rep + k;
    sim3_lm_body(P, o, lds, s_tot);
}
