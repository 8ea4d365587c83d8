// tspnp.h -- tracking::CheckMatch's cv::solvePnPRansac on the device (tsorb_match_pnp_ransac, include/tsorb.h; docs/pnpransac_recalled.md is the arithmetic).
// Three launches, no workgroup waits for another:
//   k_pnp_hyp     one hypothesis per wave (four per 256-thread workgroup): EPnP on the subset's five matches.  The 10 x 12 M, the 12 x 12 MtM and its eigenvectors
//                 live in LDS; MtM and the cyclic Jacobi iteration (round-robin order: six disjoint rotations per step) are spread over the wave's lanes, the rest
//                 runs in fp64 on lane 0 and, for the three starts of the betas, lanes 0 .. 2 (their small systems unrolled to constant indices: registers, no
//                 private memory).  Measured: 0.39 ms of the call's 0.45, whatever n (profiles/pnp_ransac_kernel_stats.txt): about nine sweeps of 11 three-barrier
//                 steps, then the serial fp64 chains
//   k_pnp_count   a thread per match, every hypothesis' pose from LDS; a count is the popcount of a wave's ballot, added as integers: exact, order-free
//   k_pnp_select  thread 0 of every workgroup walks the reference's loop (RANSACUpdateNumIters and its early stop) over the counts; the mask is the kept hypothesis
//                 evaluated again with the same arithmetic
// The per-hypothesis and per-match arithmetic is __host__ __device__ with the lane and the lane count as arguments: a host program calls it with (0, 1) and runs
// exactly what the kernel runs (the items of a phase are independent of each other, so their order does not matter).  Every loop is bounded.
#pragma once
#include "tsjacobi.h"

#define PNP_T 256
#define PNP_NW (PNP_T/64)
#define PNP_SWEEPS 40             // a 12 x 12 is diagonal after 8 - 11 sweeps; the bound only has to be finite
#define PNP_POLAR_ORTHO 1e-17     // pnp_polar3 turns a pair of columns while |g_p . g_q| > PNP_POLAR_ORTHO |g_p| |g_q|: to working precision, and no second test
#define PNP_DEGENERATE 1e-12      // scatter eigenvalue ratio below which the five points count as coplanar / collinear / coincident: the hypothesis is NaN

struct PnpWs {                    // one hypothesis' workspace: LDS on the device, the stack on the host
    double A[144], V[144];        // MtM (then its diagonal form) and the accumulated rotations: column j of V = eigenvector j
    double M[120];                // 10 x 12
    double cs[12];                // the step's six rotations (c, s)
    double pw[15], uv[10];        // the five matches
    double cw[12], al[20];        // control points (world), barycentric alphas
    double v[48];                 // v[0] .. v[3]: the eigenvectors of the four smallest eigenvalues after the basis rule
    double L[60], rho[6];
    double Rt[36], err[3];        // the three starts' R | t (3 x 4 row-major) and mean reprojection errors
    double pose[12];
};

struct PnpDev {
    int n, n_hyp; const float *Pw, *uv; const int32_t *subset; double K[4]; float thr; double confidence;
    int32_t *result, *count; double *pose, *hyp_pose; uint8_t *inlier;
};

// eigenvalues (descending, the first of equal ones first) and eigenvectors (rows of U, sign rule) of a symmetric 3 x 3: cyclic Jacobi
__host__ __device__ inline void pnp_sym3_eig(double S[3][3], double d[3], double U[3][3]) {
    double Q[3][3] = { {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0} };
#pragma unroll 1
    for (int sweep = 0; sweep < PNP_SWEEPS; sweep++) {
        if (!(fabs(S[0][1]) + fabs(S[0][2]) + fabs(S[1][2]) > 0.0)) break;
        jac_sym_rotate<3, 0, 1>(S, Q); jac_sym_rotate<3, 0, 2>(S, Q); jac_sym_rotate<3, 1, 2>(S, Q);
    }
    // descending order by three compare-and-swaps on (value, column) pairs: the first of equal ones first
    double e0 = S[0][0], e1 = S[1][1], e2 = S[2][2];
    double c0[3] = { Q[0][0], Q[1][0], Q[2][0] }, c1[3] = { Q[0][1], Q[1][1], Q[2][1] }, c2[3] = { Q[0][2], Q[1][2], Q[2][2] };
#define PNP_CSWAP(ea, ca, eb, cb) if (eb > ea) { const double t_ = ea; ea = eb; eb = t_; for (int k_ = 0; k_ < 3; k_++) { const double u_ = ca[k_]; ca[k_] = cb[k_]; cb[k_] = u_; } }
    PNP_CSWAP(e0, c0, e1, c1) PNP_CSWAP(e1, c1, e2, c2) PNP_CSWAP(e0, c0, e1, c1)
#undef PNP_CSWAP
    d[0] = e0; d[1] = e1; d[2] = e2;
#pragma unroll
    for (int k = 0; k < 3; k++) { U[0][k] = c0[k]; U[1][k] = c1[k]; U[2][k] = c2[k]; }
    jac_sign(U[0], 3); jac_sign(U[1], 3); jac_sign(U[2], 3);
}

// choose_control_points + compute_barycentric_coordinates + fill_M on the subset's five matches (one lane)
__host__ __device__ inline void pnp_setup(PnpWs &W, const float *Pw, const float *uv, const int32_t *idx, const double K[4]) {
    for (int i = 0; i < 5; i++) { const int j = idx[i];
        for (int a = 0; a < 3; a++) W.pw[3*i + a] = (double)Pw[3*j + a];
        W.uv[2*i] = (double)uv[2*j]; W.uv[2*i + 1] = (double)uv[2*j + 1]; }
    double c0[3];
    for (int a = 0; a < 3; a++) { double s = 0.0; for (int i = 0; i < 5; i++) s += W.pw[3*i + a]; c0[a] = s/5.0; }
    double S[3][3], d[3], U[3][3];
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) { double s = 0.0; for (int i = 0; i < 5; i++) s += (W.pw[3*i + a] - c0[a])*(W.pw[3*i + b] - c0[b]); S[a][b] = s; }
    pnp_sym3_eig(S, d, U);
    const bool degenerate = !(d[2] > PNP_DEGENERATE*d[0]);
    double k[3];
    for (int i = 0; i < 3; i++) k[i] = degenerate ? ts_nan() : sqrt(d[i]/5.0);
    for (int a = 0; a < 3; a++) { W.cw[a] = c0[a]; for (int i = 0; i < 3; i++) W.cw[3*(i + 1) + a] = c0[a] + k[i]*U[i][a]; }
    // CC = (k_j u_j) as columns, so row j of its inverse is u_j / k_j
    for (int i = 0; i < 5; i++) { double *a = W.al + 4*i;
        for (int j = 0; j < 3; j++) a[1 + j] = ((U[j][0]/k[j])*(W.pw[3*i] - c0[0]) + (U[j][1]/k[j])*(W.pw[3*i + 1] - c0[1])) + (U[j][2]/k[j])*(W.pw[3*i + 2] - c0[2]);
        a[0] = 1.0 - a[1] - a[2] - a[3]; }
    for (int i = 0; i < 5; i++) { double *M1 = W.M + 24*i, *M2 = M1 + 12; const double *a = W.al + 4*i, u = W.uv[2*i], v = W.uv[2*i + 1];
        for (int j = 0; j < 4; j++) { M1[3*j] = a[j]*K[0]; M1[3*j + 1] = 0.0; M1[3*j + 2] = a[j]*(K[2] - u);
                                      M2[3*j] = 0.0; M2[3*j + 1] = a[j]*K[1]; M2[3*j + 2] = a[j]*(K[3] - v); } }
}

// A = MtM, V = I (lanes)
__host__ __device__ inline void pnp_mtm(PnpWs &W, int lane, int nl) {
    for (int e = lane; e < 144; e += nl) { const int i = e/12, j = e%12; double s = 0.0;
        for (int r = 0; r < 10; r++) s += W.M[12*r + i]*W.M[12*r + j];
        W.A[e] = s; W.V[e] = i == j ? 1.0 : 0.0; }
}

// cyclic Jacobi on the symmetric 12 x 12 in W.A: A <- J^T A J, V <- V J, the six disjoint rotations of a round-robin step over 12 indices (jac_pair<11>) at a time (lanes)
__host__ __device__ inline void pnp_jacobi12(PnpWs &W, int lane, int nl) {
#pragma unroll 1
    for (int sweep = 0; sweep < PNP_SWEEPS; sweep++) {
        double off = 0.0;
        for (int i = 0; i < 12; i++) for (int j = i + 1; j < 12; j++) off += fabs(W.A[12*i + j]);
        if (TS_ALL(!(off > 0.0))) break;                                   // diagonal (or NaN: nothing to gain); uniform over the workgroup
#pragma unroll 1
        for (int r = 0; r < 11; r++) {
            for (int i = lane; i < 6; i += nl) { int p, q; jac_pair<11>(r, i, p, q);
                jac_sym_rotation(W.A[13*p], W.A[13*q], W.A[12*p + q], W.cs[2*i], W.cs[2*i + 1]); }
            TS_BARRIER();
            for (int e = lane; e < 144; e += nl) { const int i = (e%72)/12, k = e%12; int p, q; jac_pair<11>(r, i, p, q);
                double *X = e < 72 ? W.A : W.V; const double c = W.cs[2*i], s = W.cs[2*i + 1];
                const double xkp = X[12*k + p], xkq = X[12*k + q]; X[12*k + p] = c*xkp - s*xkq; X[12*k + q] = s*xkp + c*xkq; }
            TS_BARRIER();
            for (int e = lane; e < 72; e += nl) { const int i = e/12, k = e%12; int p, q; jac_pair<11>(r, i, p, q);
                const double c = W.cs[2*i], s = W.cs[2*i + 1];
                const double apk = W.A[12*p + k], aqk = W.A[12*q + k];
                W.A[12*p + k] = k == q ? 0.0 : c*apk - s*aqk; W.A[12*q + k] = k == p ? 0.0 : s*apk + c*aqk; }
            TS_BARRIER();
        }
    }
}

// the eigenvectors of the four smallest eigenvalues (v[0] the smallest), the basis rule on the null pair, signs; compute_L_6x10 and compute_rho (one lane)
__host__ __device__ inline void pnp_basis(PnpWs &W) {
    int o[12];
    for (int i = 0; i < 12; i++) o[i] = i;
    for (int i = 1; i < 12; i++) for (int j = i; j > 0 && W.A[13*o[j]] < W.A[13*o[j - 1]]; j--) { const int t = o[j]; o[j] = o[j - 1]; o[j - 1] = t; }
    for (int m = 0; m < 4; m++) for (int j = 0; j < 12; j++) W.v[12*m + j] = W.V[12*j + o[m]];
    double *v0 = W.v, *v1 = W.v + 12;
    int k = 0; double best = v0[0]*v0[0] + v1[0]*v1[0];
    for (int j = 1; j < 12; j++) { const double pj = v0[j]*v0[j] + v1[j]*v1[j]; if (pj > best) { best = pj; k = j; } }
    const double a = v0[k], b = v1[k], rr = sqrt(a*a + b*b);
    for (int j = 0; j < 12; j++) { const double x = v0[j], y = v1[j]; v1[j] = (a*x + b*y)/rr; v0[j] = (b*x - a*y)/rr; }
    jac_sign(v0, 12); jac_sign(W.v + 24, 12); jac_sign(W.v + 36, 12);
    double (*dv)[6][3] = (double (*)[6][3])W.M;                               // 72 doubles in M's place (MtM has been formed)
    for (int i = 0; i < 4; i++) { int p = 0, q = 1; const double *v = W.v + 12*i;
        for (int j = 0; j < 6; j++) { for (int c = 0; c < 3; c++) dv[i][j][c] = v[3*p + c] - v[3*q + c];
            q++; if (q > 3) { p++; q = p + 1; } } }
#define PNP_DOT(x, y) ((x[0]*y[0] + x[1]*y[1]) + x[2]*y[2])
    for (int i = 0; i < 6; i++) { double *row = W.L + 10*i;
        row[0] = PNP_DOT(dv[0][i], dv[0][i]); row[1] = 2.0*PNP_DOT(dv[0][i], dv[1][i]); row[2] = PNP_DOT(dv[1][i], dv[1][i]);
        row[3] = 2.0*PNP_DOT(dv[0][i], dv[2][i]); row[4] = 2.0*PNP_DOT(dv[1][i], dv[2][i]); row[5] = PNP_DOT(dv[2][i], dv[2][i]);
        row[6] = 2.0*PNP_DOT(dv[0][i], dv[3][i]); row[7] = 2.0*PNP_DOT(dv[1][i], dv[3][i]); row[8] = 2.0*PNP_DOT(dv[2][i], dv[3][i]);
        row[9] = PNP_DOT(dv[3][i], dv[3][i]); }
    { int p = 0, q = 1;
      for (int j = 0; j < 6; j++) { double s = 0.0;
          for (int c = 0; c < 3; c++) { const double d = W.cw[3*p + c] - W.cw[3*q + c]; s += d*d; }
          W.rho[j] = s; q++; if (q > 3) { p++; q = p + 1; } } }
}

// least squares of the 6 x nc system in the first nc of NC columns (the others are zero) by Householder reflections; x[j] = 0 for j >= nc; a rank-deficient system
// gives non-finite values.  Every index is a constant after unrolling, so the system stays in registers; a lane with a smaller nc idles through the steps it skips.
template <int NC>
__host__ __device__ __forceinline__ void pnp_lstsq6(double (&A)[6][NC], int nc, double (&b)[6], double (&x)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; k++) {
        if (k < nc) {
            double nrm = 0.0;
#pragma unroll
            for (int i = k; i < 6; i++) nrm += A[i][k]*A[i][k];
            nrm = sqrt(nrm);
            const double alpha = A[k][k] > 0.0 ? -nrm : nrm;
            double v[6], vv = 0.0;
#pragma unroll
            for (int i = k; i < 6; i++) { v[i] = A[i][k] - (i == k ? alpha : 0.0); vv += v[i]*v[i]; }
#pragma unroll
            for (int j = k + 1; j < NC; j++) { double s = 0.0;
#pragma unroll
                for (int i = k; i < 6; i++) s += v[i]*A[i][j];
                const double f = 2.0*s/vv;
#pragma unroll
                for (int i = k; i < 6; i++) A[i][j] -= f*v[i]; }
            { double s = 0.0;
#pragma unroll
              for (int i = k; i < 6; i++) s += v[i]*b[i];
              const double f = 2.0*s/vv;
#pragma unroll
              for (int i = k; i < 6; i++) b[i] -= f*v[i]; }
            A[k][k] = alpha;
        }
    }
#pragma unroll
    for (int k = NC - 1; k >= 0; k--) { double s = b[k];
#pragma unroll
        for (int j = k + 1; j < NC; j++) s -= A[k][j]*x[j];
        x[k] = k < nc ? s/A[k][k] : 0.0; }
}

// R = U V^T of the 3 x 3 B = U S V^T by one-sided Jacobi (the columns of B turned until they are orthogonal): independent of the order and signs of the triplets
__host__ __device__ inline void pnp_polar3(const double B[3][3], double R[3][3]) {
    double G[3][3], Q[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = B[i][j];
    jac_orthogonalize(G, Q, PNP_POLAR_ORTHO, 0.0);
#pragma unroll
    for (int j = 0; j < 3; j++) { const double nrm = sqrt(jac_length2(G, j));
#pragma unroll
        for (int i = 0; i < 3; i++) G[i][j] /= nrm; }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = (G[i][0]*Q[j][0] + G[i][1]*Q[j][1]) + G[i][2]*Q[j][2];
}

// start s of the betas (find_betas_approx_1 / _2 / _3), five Gauss-Newton steps, compute_R_and_t: W.Rt[12 s ..], W.err[s] (one lane per start)
__host__ __device__ inline void pnp_start(PnpWs &W, const double K[4], int s) {
    const int nc = s == 0 ? 4 : (s == 1 ? 3 : 5);
    double be[4], b[6];
    {   double A[6][5], x[5];
#pragma unroll
        for (int i = 0; i < 6; i++) { const double *row = W.L + 10*i; b[i] = W.rho[i];
            A[i][0] = row[0]; A[i][1] = row[1]; A[i][2] = s == 0 ? row[3] : row[2]; A[i][3] = s == 0 ? row[6] : (s == 2 ? row[3] : 0.0); A[i][4] = s == 2 ? row[4] : 0.0; }
        pnp_lstsq6<5>(A, nc, b, x);
        if (s == 0) {
            if (x[0] < 0.0) { be[0] = sqrt(-x[0]); be[1] = -x[1]/be[0]; be[2] = -x[2]/be[0]; be[3] = -x[3]/be[0]; }
            else { be[0] = sqrt(x[0]); be[1] = x[1]/be[0]; be[2] = x[2]/be[0]; be[3] = x[3]/be[0]; }
        } else {
            if (x[0] < 0.0) { be[0] = sqrt(-x[0]); be[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0; }
            else { be[0] = sqrt(x[0]); be[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0; }
            if (x[1] < 0.0) be[0] = -be[0];
            be[2] = s == 2 ? x[3]/be[0] : 0.0; be[3] = 0.0;
        }
    }
#pragma unroll 1
    for (int it = 0; it < 5; it++) {
        double A[6][4], x[4];
#pragma unroll
        for (int i = 0; i < 6; i++) { const double *l = W.L + 10*i;
            A[i][0] = 2.0*l[0]*be[0] + l[1]*be[1] + l[3]*be[2] + l[6]*be[3];
            A[i][1] = l[1]*be[0] + 2.0*l[2]*be[1] + l[4]*be[2] + l[7]*be[3];
            A[i][2] = l[3]*be[0] + l[4]*be[1] + 2.0*l[5]*be[2] + l[8]*be[3];
            A[i][3] = l[6]*be[0] + l[7]*be[1] + l[8]*be[2] + 2.0*l[9]*be[3];
            b[i] = W.rho[i] - (l[0]*be[0]*be[0] + l[1]*be[0]*be[1] + l[2]*be[1]*be[1] + l[3]*be[0]*be[2] + l[4]*be[1]*be[2] + l[5]*be[2]*be[2]
                               + l[6]*be[0]*be[3] + l[7]*be[1]*be[3] + l[8]*be[2]*be[3] + l[9]*be[3]*be[3]); }
        pnp_lstsq6<4>(A, 4, b, x);
        be[0] += x[0]; be[1] += x[1]; be[2] += x[2]; be[3] += x[3];
    }
    // compute_ccs, compute_pcs, solve_for_sign
    double cc[12], pc[15];
    for (int j = 0; j < 12; j++) cc[j] = ((be[0]*W.v[j] + be[1]*W.v[12 + j]) + be[2]*W.v[24 + j]) + be[3]*W.v[36 + j];
    for (int i = 0; i < 5; i++) { const double *a = W.al + 4*i;
        for (int c = 0; c < 3; c++) pc[3*i + c] = ((a[0]*cc[c] + a[1]*cc[3 + c]) + a[2]*cc[6 + c]) + a[3]*cc[9 + c]; }
    if (pc[2] < 0.0) for (int j = 0; j < 15; j++) pc[j] = -pc[j];
    // estimate_R_and_t
    double pc0[3], pw0[3], B[3][3], R[3][3], t[3];
    for (int c = 0; c < 3; c++) { double sc = 0.0, sw = 0.0; for (int i = 0; i < 5; i++) { sc += pc[3*i + c]; sw += W.pw[3*i + c]; } pc0[c] = sc/5.0; pw0[c] = sw/5.0; }
    for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) { double sum = 0.0; for (int i = 0; i < 5; i++) sum += (pc[3*i + j] - pc0[j])*(W.pw[3*i + k] - pw0[k]); B[j][k] = sum; }
    pnp_polar3(B, R);
    const double det = (R[0][0]*R[1][1]*R[2][2] + R[0][1]*R[1][2]*R[2][0] + R[0][2]*R[1][0]*R[2][1]) - (R[0][2]*R[1][1]*R[2][0] + R[0][1]*R[1][0]*R[2][2] + R[0][0]*R[1][2]*R[2][1]);
    if (det < 0.0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
    for (int c = 0; c < 3; c++) t[c] = pc0[c] - ((R[c][0]*pw0[0] + R[c][1]*pw0[1]) + R[c][2]*pw0[2]);
    // reprojection_error
    double sum = 0.0;
    for (int i = 0; i < 5; i++) { const double *p = W.pw + 3*i;
        const double Xc = ((R[0][0]*p[0] + R[0][1]*p[1]) + R[0][2]*p[2]) + t[0], Yc = ((R[1][0]*p[0] + R[1][1]*p[1]) + R[1][2]*p[2]) + t[1];
        const double iz = 1.0/(((R[2][0]*p[0] + R[2][1]*p[1]) + R[2][2]*p[2]) + t[2]);
        const double du = W.uv[2*i] - (K[2] + K[0]*Xc*iz), dv = W.uv[2*i + 1] - (K[3] + K[1]*Yc*iz);
        sum += sqrt(du*du + dv*dv); }
    W.err[s] = sum/5.0;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) W.Rt[12*s + 4*r + c] = R[r][c]; W.Rt[12*s + 4*r + 3] = t[r]; }
}

// epnp::compute_pose on the subset: W.pose = R | t (3 x 4 row-major) of the start with the smallest error, in the reference's order of comparisons
__host__ __device__ inline void pnp_hypothesis(PnpWs &W, const float *Pw, const float *uv, const int32_t *idx, const double K[4], int lane, int nl) {
    if (lane == 0) pnp_setup(W, Pw, uv, idx, K);
    TS_BARRIER();
    pnp_mtm(W, lane, nl);
    TS_BARRIER();
    pnp_jacobi12(W, lane, nl);
    if (lane == 0) pnp_basis(W);
    TS_BARRIER();
    for (int s = lane; s < 3; s += nl) pnp_start(W, K, s);
    TS_BARRIER();
    if (lane == 0) { int N = 0;
        if (W.err[1] < W.err[0]) N = 1;
        if (W.err[2] < W.err[N]) N = 2;
        for (int j = 0; j < 12; j++) W.pose[j] = W.Rt[12*N + j]; }
    TS_BARRIER();
}

// PnPRansacCallback::computeError for one match: projectPoints in double stored as float, float differences, their squares added in float
__host__ __device__ __forceinline__ float pnp_err(const double *T, const double K[4], const float P[3], const float uv[2]) {
    const double X = ((T[0]*P[0] + T[1]*P[1]) + T[2]*P[2]) + T[3], Y = ((T[4]*P[0] + T[5]*P[1]) + T[6]*P[2]) + T[7], Z = ((T[8]*P[0] + T[9]*P[1]) + T[10]*P[2]) + T[11];
    const double iz = Z != 0.0 ? 1.0/Z : 1.0;
    const float u = (float)((X*iz)*K[0] + K[2]), v = (float)((Y*iz)*K[1] + K[3]);
    const float du = uv[0] - u, dv = uv[1] - v;
    return du*du + dv*dv;
}
__host__ __device__ __forceinline__ bool pnp_inlier(const double *T, const double K[4], const float P[3], const float uv[2], float thr) { return pnp_err(T, K, P, uv) <= thr; }     // (a NaN compares false)

// RANSACUpdateNumIters(p, ep, 5, max_iters); cvRound = round half to even
__host__ __device__ inline int pnp_update_iters(double p, double ep, int max_iters) {
    p = fmax(p, 0.0); p = fmin(p, 1.0); ep = fmax(ep, 0.0); ep = fmin(ep, 1.0);
    double num = fmax(1.0 - p, 2.2250738585072014e-308), denom = 1.0 - pow(1.0 - ep, 5.0);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num); denom = log(denom);
    return denom >= 0.0 || -num >= max_iters*(-denom) ? max_iters : (int)rint(num/denom);
}

// RANSACPointSetRegistrator::run's loop over the counts: result = ok, n_inlier, sel, n_run
__host__ __device__ inline void pnp_walk(const int32_t *count, int n_hyp, int n, double confidence, int32_t result[4]) {
    int max_good = 0, best = -1, niters = n_hyp, iter = 0;
    for (; iter < niters; iter++) {                                         // niters only ever shrinks: bounded by n_hyp
        const int c = count[iter];
        if (c > (max_good > 4 ? max_good : 4)) { best = iter; max_good = c; niters = pnp_update_iters(confidence, (double)(n - c)/n, niters); }
    }
    result[0] = max_good > 0 ? 1 : 0; result[1] = max_good; result[2] = best; result[3] = iter;
}

__global__ __launch_bounds__(PNP_T) void k_pnp_hyp(PnpDev D) {
    __shared__ PnpWs ws[PNP_NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x*PNP_NW + wave, hh = h < D.n_hyp ? h : D.n_hyp - 1;     // a wave past the end repeats the last hypothesis: the barriers stay whole
    pnp_hypothesis(ws[wave], D.Pw, D.uv, D.subset + 5*hh, D.K, lane, 64);
    if (h < D.n_hyp) { if (lane < 12) D.hyp_pose[12*(size_t)h + lane] = ws[wave].pose[lane];
        if (lane == 12) D.count[h] = 0; }
}

__global__ __launch_bounds__(PNP_T) void k_pnp_count(PnpDev D) {
    __shared__ double s_pose[TSORB_PNP_MAX_HYP*12];
    __shared__ int s_cnt[PNP_NW][TSORB_PNP_MAX_HYP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, H = D.n_hyp;
    for (int j = tid; j < 12*H; j += PNP_T) s_pose[j] = D.hyp_pose[j];
    for (int j = tid; j < PNP_NW*TSORB_PNP_MAX_HYP; j += PNP_T) (&s_cnt[0][0])[j] = 0;
    __syncthreads();
    const int i = blockIdx.x*PNP_T + tid; const bool have = i < D.n; const int j = have ? i : 0;
    const float P[3] = { D.Pw[3*j], D.Pw[3*j + 1], D.Pw[3*j + 2] }, q[2] = { D.uv[2*j], D.uv[2*j + 1] };
#pragma unroll 1
    for (int h = 0; h < H; h++) {                                           // the same trip count for every thread: a wave's ballot is whole
        const bool in = have && pnp_inlier(s_pose + 12*h, D.K, P, q, D.thr);
        const unsigned long long b = __ballot(in);
        if (lane == 0) s_cnt[wave][h] = __popcll(b);
    }
    __syncthreads();
    for (int h = tid; h < H; h += PNP_T) { int c = 0;
        for (int w = 0; w < PNP_NW; w++) c += s_cnt[w][h];
        if (c) atomicAdd(D.count + h, c); }
}

__global__ __launch_bounds__(PNP_T) void k_pnp_select(PnpDev D) {
    __shared__ int s_res[4];
    __shared__ double s_pose[12];
    const int tid = threadIdx.x;
    if (tid == 0) { int32_t r[4]; pnp_walk(D.count, D.n_hyp, D.n, D.confidence, r);
        for (int j = 0; j < 4; j++) s_res[j] = r[j];
        if (blockIdx.x == 0) for (int j = 0; j < 4; j++) D.result[j] = r[j]; }
    __syncthreads();
    const bool ok = s_res[0] != 0; const int sel = s_res[2];
    if (tid < 12) { const double v = ok ? D.hyp_pose[12*(size_t)sel + tid] : 0.0; s_pose[tid] = v; if (blockIdx.x == 0) D.pose[tid] = v; }
    __syncthreads();
    const int i = blockIdx.x*PNP_T + tid;
    if (i < D.n) { const float P[3] = { D.Pw[3*i], D.Pw[3*i + 1], D.Pw[3*i + 2] }, q[2] = { D.uv[2*i], D.uv[2*i + 1] };
        D.inlier[i] = (ok && pnp_inlier(s_pose, D.K, P, q, D.thr)) ? 1 : 0; }
}
