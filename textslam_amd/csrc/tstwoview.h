// tstwoview.h -- initializer::FindHomography / FindFundamental on the device (tsorb_match_two_view_ransac, include/tsorb.h; docs/twoview_recalled.md is the arithmetic).
// Three launches, no workgroup waits for another:
//   k_tv_fit     one fit per wave and workgroup, 2 n_hyp fits: the H fits first, then the F fits.  The 16 x 9 (H) or 8 x 9 (F) system A and the
//                accumulated rotations V live in LDS; the null vector is the right singular vector of A's smallest singular value by a one-sided (Hestenes) Jacobi
//                iteration on A's nine columns in fp64 -- the round-robin order over 9 indices and a bye (9 steps of 4 disjoint pairs a sweep), a lane per pair for
//                the rotation, a lane per (pair, row) for turning A and V.  Lane 0 then forms the model (F: the 3 x 3 by the same iteration in registers, its
//                smallest singular value set to 0) and rounds it to float ONCE.
//   k_tv_score   one (model, hypothesis) per wave: the lanes form the two float terms of 64 matches at a time, and every lane adds the 128 terms in the reference's
//                order (match by match, first term then second) from v_readlane: a serial chain of 2 n float adds, the same bits as the host loop.
//   k_tv_select  one workgroup: the scores go to LDS, lane 0 of waves 0 and 1 run the two keep loops over them (strictly greater from 0.0: the first of equal scores stays, a NaN is never kept),
//                then all threads re-form the kept hypotheses' masks with the same device functions.
// Everything that decides anything is __host__ __device__ with the lane and the lane count as arguments: a host program calls it with (0, 1) and runs what the kernel
// runs (the items of a phase are independent of each other).  Every loop is bounded.  Float arithmetic whose bits matter goes through tsjacobi.h's TS_FMUL / TS_FADD / TS_FSUB /
// TS_FDIV: one rounding each, no contraction (the library and the host builds also use -ffp-contract=off).
#pragma once
#pragma clang fp contract(off)
#include "tsjacobi.h"

#define TV_T 256
#define TV_NW (TV_T/64)
#define TV_SWEEPS 40              // nine columns are orthogonal after 6 - 9 sweeps; the bound only has to be finite
#define TV_DEGENERATE 1e-12       // second smallest eigenvalue of AtA over the largest at or below which the subset is degenerate: the model is NaN

struct TvWs {                     // one fit's workspace: LDS on the device, the stack on the host
    double A[144], V[81];         // the system (16 or 8 rows of 9) and the accumulated rotations: A_now = A_0 V
    double cs[10];                // the step's rotations (c, s) of pairs 1 .. 4 (pair 0 is the bye)
    int flag[8];                  // pair i turned in this sweep
    int sweeps;                   // sweeps the iteration ran, the last one (in which nothing turned) included: diagnostics
    float model[9];               // H21i or F21i
};

struct TvDev {
    int n, n_hyp; const float *xy1, *xy2; const int32_t *subset; float norm1[4], norm2[4], sigma;
    float *hyp_score, *hyp_model, *score, *model; int32_t *sel; uint8_t *inl_h, *inl_f;
};

// initializer::Normalize's point: (x - mean) * s, two float roundings
__host__ __device__ __forceinline__ float tv_normalized(float x, float mean, float s) { return TS_FMUL(TS_FSUB(x, mean), s); }

// ComputeH21's 16 x 9 (model 0) or ComputeF21's 8 x 9 (model 1) from the subset's eight matches: the reference's float products, then doubles; V = I (lanes)
__host__ __device__ inline void tv_setup(TvWs &W, int model, const float *xy1, const float *xy2, const float *n1, const float *n2, const int32_t *idx, int lane, int nl) {
    for (int j = lane; j < 8; j += nl) { const int i = idx[j];
        const float u1 = tv_normalized(xy1[2*i], n1[0], n1[2]), v1 = tv_normalized(xy1[2*i + 1], n1[1], n1[3]);
        const float u2 = tv_normalized(xy2[2*i], n2[0], n2[2]), v2 = tv_normalized(xy2[2*i + 1], n2[1], n2[3]);
        if (model == 0) { double *a = W.A + 18*j, *b = a + 9;
            a[0] = 0.0; a[1] = 0.0; a[2] = 0.0; a[3] = (double)-u1; a[4] = (double)-v1; a[5] = -1.0;
            a[6] = (double)TS_FMUL(v2, u1); a[7] = (double)TS_FMUL(v2, v1); a[8] = (double)v2;
            b[0] = (double)u1; b[1] = (double)v1; b[2] = 1.0; b[3] = 0.0; b[4] = 0.0; b[5] = 0.0;
            b[6] = (double)TS_FMUL(-u2, u1); b[7] = (double)TS_FMUL(-u2, v1); b[8] = (double)-u2;
        } else { double *a = W.A + 9*j;
            a[0] = (double)TS_FMUL(u2, u1); a[1] = (double)TS_FMUL(u2, v1); a[2] = (double)u2;
            a[3] = (double)TS_FMUL(v2, u1); a[4] = (double)TS_FMUL(v2, v1); a[5] = (double)v2;
            a[6] = (double)u1; a[7] = (double)v1; a[8] = 1.0; } }
    for (int e = lane; e < 81; e += nl) W.V[e] = e/9 == e%9 ? 1.0 : 0.0;
}

// one-sided Jacobi on the m x 9 in W.A: its columns turned until they are orthogonal, V <- V J, the four disjoint pairs i = 1 .. 4 of a round-robin step over 9 indices
// and a bye (jac_pair<9>) at a time (lanes)
__host__ __device__ inline void tv_jacobi9(TvWs &W, int m, int lane, int nl) {
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SWEEPS; sweep++) {
        for (int i = 1 + lane; i < 5; i += nl) W.flag[i] = 0;
#pragma unroll 1
        for (int r = 0; r < 9; r++) {
            for (int i = 1 + lane; i < 5; i += nl) { int p, q; jac_pair<9>(r, i, p, q);
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int k = 0; k < m; k++) { const double ap = W.A[9*k + p], aq = W.A[9*k + q]; al += ap*ap; be += aq*aq; ga += ap*aq; }
                if (jac_rotation(al, be, ga, JAC_ORTHO, JAC_TINY, W.cs[2*i], W.cs[2*i + 1])) W.flag[i] = 1; }
            TS_BARRIER();
            for (int e = lane; e < 4*(m + 9); e += nl) { const int i = 1 + e/(m + 9), k = e%(m + 9); int p, q; jac_pair<9>(r, i, p, q);
                double *X = k < m ? W.A + 9*k : W.V + 9*(k - m); const double c = W.cs[2*i], s = W.cs[2*i + 1];
                const double xp = X[p], xq = X[q]; X[p] = c*xp - s*xq; X[q] = s*xp + c*xq; }
            TS_BARRIER();
        }
        const bool any = (W.flag[1] | W.flag[2] | W.flag[3] | W.flag[4]) != 0;
        if (lane == 0) W.sweeps = sweep + 1;
        if (TS_ALL(!any)) break;                                            // nothing turned in a whole sweep (a NaN never turns); uniform over the workgroup
    }
}

// the unit right singular vector of the smallest singular value (the first of equal ones), sign rule; NaN when the subset is degenerate (one lane)
__host__ __device__ inline void tv_null_vector(const TvWs &W, int m, double v[9]) {
    double d[9];
    for (int j = 0; j < 9; j++) { double s = 0.0; for (int k = 0; k < m; k++) s += W.A[9*k + j]*W.A[9*k + j]; d[j] = s; }
    int jmin = 0;
    for (int j = 1; j < 9; j++) if (d[j] < d[jmin]) jmin = j;
    double dmax = d[0], d2 = -1.0;
    for (int j = 0; j < 9; j++) { if (d[j] > dmax) dmax = d[j]; if (j != jmin && (d2 < 0.0 || d[j] < d2)) d2 = d[j]; }
    const bool degenerate = !(d2 > TV_DEGENERATE*dmax);
    double nn = 0.0;
    for (int j = 0; j < 9; j++) { v[j] = W.V[9*j + jmin]; nn += v[j]*v[j]; }
    nn = sqrt(nn);
    for (int j = 0; j < 9; j++) v[j] = degenerate ? ts_nan() : v[j]/nn;
    jac_sign(v, 9);
}

// ComputeF21's second SVD: F = U diag(w) V^T with the smallest w (the first of equal ones) set to 0.  G = F Q has orthogonal columns u_j w_j, so the answer is
// G with that column zeroed, times Q^T: independent of the order and signs of the triplets
__host__ __device__ inline void tv_rank2(const double F[9], double Fn[9]) {
    double G[3][3], Q[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = F[3*i + j];
    jac_orthogonalize(G, Q, JAC_ORTHO, JAC_TINY);
    const int jmin = jac_shortest(G);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Fn[3*i + j] = ((jmin == 0 ? 0.0 : G[i][0]*Q[j][0]) + (jmin == 1 ? 0.0 : G[i][1]*Q[j][1])) + (jmin == 2 ? 0.0 : G[i][2]*Q[j][2]);
}

// T = [[sX, 0, -meanX sX], [0, sY, -meanY sY], [0, 0, 1]] as the reference's floats: t[0 .. 3] = sX, sY, T02, T12
__host__ __device__ __forceinline__ void tv_T(const float nrm[4], double t[4]) {
    t[0] = (double)nrm[2]; t[1] = (double)nrm[3]; t[2] = (double)TS_FMUL(-nrm[0], nrm[2]); t[3] = (double)TS_FMUL(-nrm[1], nrm[3]);
}

// M T1 for a 3 x 3 M (fp64)
__host__ __device__ __forceinline__ void tv_times_T(const double M[9], const double t1[4], double out[9]) {
    for (int r = 0; r < 3; r++) { out[3*r] = M[3*r]*t1[0]; out[3*r + 1] = M[3*r + 1]*t1[1]; out[3*r + 2] = (M[3*r]*t1[2] + M[3*r + 1]*t1[3]) + M[3*r + 2]; }
}

// the model of the fit in W: H21i = T2^-1 Hn T1 or F21i = T2^T Fn T1, fp64 from A on, rounded to float once (one lane)
__host__ __device__ inline void tv_model(TvWs &W, int model, const float *n1, const float *n2) {
    double v[9], M[9], out[9], t1[4], t2[4];
    tv_null_vector(W, model == 0 ? 16 : 8, v);
    tv_T(n1, t1); tv_T(n2, t2);
    if (model == 0) {                                                       // T2^-1 = [[1/sX, 0, -T02/sX], [0, 1/sY, -T12/sY], [0, 0, 1]]
        const double i00 = 1.0/t2[0], i02 = -t2[2]/t2[0], i11 = 1.0/t2[1], i12 = -t2[3]/t2[1];
        for (int c = 0; c < 3; c++) { M[c] = i00*v[c] + i02*v[6 + c]; M[3 + c] = i11*v[3 + c] + i12*v[6 + c]; M[6 + c] = v[6 + c]; }
    } else {
        double Fn[9]; tv_rank2(v, Fn);
        for (int c = 0; c < 3; c++) { M[c] = t2[0]*Fn[c]; M[3 + c] = t2[1]*Fn[3 + c]; M[6 + c] = (t2[2]*Fn[c] + t2[3]*Fn[3 + c]) + Fn[6 + c]; }
    }
    tv_times_T(M, t1, out);
    for (int j = 0; j < 9; j++) W.model[j] = (float)out[j];
}

__host__ __device__ inline void tv_fit(TvWs &W, int model, const float *xy1, const float *xy2, const float *n1, const float *n2, const int32_t *idx, int lane, int nl) {
    tv_setup(W, model, xy1, xy2, n1, n2, idx, lane, nl);
    TS_BARRIER();
    tv_jacobi9(W, model == 0 ? 16 : 8, lane, nl);
    if (lane == 0) tv_model(W, model, n1, n2);
    TS_BARRIER();
}

// H12i = the inverse of the FLOAT H21i: adjugate over determinant in fp64, rounded to float; a zero determinant gives zeros (cv::Mat::inv() as recalled)
__host__ __device__ inline void tv_h_inverse(const float h[9], float hi[9]) {
    const double a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7], l = h[8];
    const double adj[9] = { e*l - f*k, c*k - b*l, b*f - c*e, f*g - d*l, a*l - c*g, c*d - a*f, d*k - e*g, b*g - a*k, a*e - b*d };
    const double det = (a*adj[0] + b*adj[3]) + c*adj[6];
    for (int j = 0; j < 9; j++) hi[j] = det == 0.0 ? 0.f : (float)(adj[j]/det);
}

__host__ __device__ __forceinline__ float tv_inv_sigma2(float sigma) { return (float)(1.0/(double)TS_FMUL(sigma, sigma)); }
__host__ __device__ __forceinline__ float tv_dot3(float a, float x, float b, float y, float c) { return TS_FADD(TS_FADD(TS_FMUL(a, x), TS_FMUL(b, y)), c); }

// CheckHomography for one match: the two score terms (0 where the reference adds nothing; a term is never negative, so adding it changes no bit) and bIn
__host__ __device__ inline bool tv_terms_h(const float *h, const float *hi, float u1, float v1, float u2, float v2, float iss, float &t1, float &t2) {
    const float th = 5.991f; bool in = true;
    const float w2 = (float)(1.0/(double)tv_dot3(hi[6], u2, hi[7], v2, hi[8]));
    const float u2in1 = TS_FMUL(tv_dot3(hi[0], u2, hi[1], v2, hi[2]), w2), v2in1 = TS_FMUL(tv_dot3(hi[3], u2, hi[4], v2, hi[5]), w2);
    const float du1 = TS_FSUB(u1, u2in1), dv1 = TS_FSUB(v1, v2in1);
    const float chi1 = TS_FMUL(TS_FADD(TS_FMUL(du1, du1), TS_FMUL(dv1, dv1)), iss);
    if (chi1 > th) { in = false; t1 = 0.f; } else t1 = TS_FSUB(th, chi1);
    const float w1 = (float)(1.0/(double)tv_dot3(h[6], u1, h[7], v1, h[8]));
    const float u1in2 = TS_FMUL(tv_dot3(h[0], u1, h[1], v1, h[2]), w1), v1in2 = TS_FMUL(tv_dot3(h[3], u1, h[4], v1, h[5]), w1);
    const float du2 = TS_FSUB(u2, u1in2), dv2 = TS_FSUB(v2, v1in2);
    const float chi2 = TS_FMUL(TS_FADD(TS_FMUL(du2, du2), TS_FMUL(dv2, dv2)), iss);
    if (chi2 > th) { in = false; t2 = 0.f; } else t2 = TS_FSUB(th, chi2);
    return in;
}

// CheckFundamental for one match
__host__ __device__ inline bool tv_terms_f(const float *f, float u1, float v1, float u2, float v2, float iss, float &t1, float &t2) {
    const float th = 3.841f, thScore = 5.991f; bool in = true;
    const float a2 = tv_dot3(f[0], u1, f[1], v1, f[2]), b2 = tv_dot3(f[3], u1, f[4], v1, f[5]), c2 = tv_dot3(f[6], u1, f[7], v1, f[8]);
    const float num2 = tv_dot3(a2, u2, b2, v2, c2);
    const float chi1 = TS_FMUL(TS_FDIV(TS_FMUL(num2, num2), TS_FADD(TS_FMUL(a2, a2), TS_FMUL(b2, b2))), iss);
    if (chi1 > th) { in = false; t1 = 0.f; } else t1 = TS_FSUB(thScore, chi1);
    const float a1 = tv_dot3(f[0], u2, f[3], v2, f[6]), b1 = tv_dot3(f[1], u2, f[4], v2, f[7]), c1 = tv_dot3(f[2], u2, f[5], v2, f[8]);
    const float num1 = tv_dot3(a1, u1, b1, v1, c1);
    const float chi2 = TS_FMUL(TS_FDIV(TS_FMUL(num1, num1), TS_FADD(TS_FMUL(a1, a1), TS_FMUL(b1, b1))), iss);
    if (chi2 > th) { in = false; t2 = 0.f; } else t2 = TS_FSUB(thScore, chi2);
    return in;
}

__host__ __device__ __forceinline__ bool tv_terms(int model, const float *m, const float *hi, const float *p1, const float *p2, float iss, float &t1, float &t2) {
    return model == 0 ? tv_terms_h(m, hi, p1[0], p1[1], p2[0], p2[1], iss, t1, t2) : tv_terms_f(m, p1[0], p1[1], p2[0], p2[1], iss, t1, t2);
}

// a hypothesis' score as the reference's loop forms it: the sequential float sum over the matches in index order, first term then second.  mask may be NULL
__host__ __device__ inline float tv_score_serial(int model, const float *m, int n, const float *xy1, const float *xy2, float sigma, uint8_t *mask) {
    float hi[9] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, s = 0.f; const float iss = tv_inv_sigma2(sigma);
    if (model == 0) tv_h_inverse(m, hi);
    for (int i = 0; i < n; i++) { float t1, t2; const bool in = tv_terms(model, m, hi, xy1 + 2*i, xy2 + 2*i, iss, t1, t2);
        s = TS_FADD(s, t1); s = TS_FADD(s, t2);
        if (mask) mask[i] = in ? 1 : 0; }
    return s;
}

// FindHomography's / FindFundamental's keep loop: from 0.0, strictly greater (a NaN compares false); -1 = nothing kept
__host__ __device__ inline int tv_keep(const float *score, int n_hyp, float &best) {
    int sel = -1; best = 0.f;
    for (int h = 0; h < n_hyp; h++) if (score[h] > best) { best = score[h]; sel = h; }
    return sel;
}

__global__ __launch_bounds__(64) void k_tv_fit(TvDev D) {             // one wave per workgroup: the barriers of the iteration are this fit's alone, and it stops when IT is done
    __shared__ TvWs ws;
    const int lane = threadIdx.x, g = blockIdx.x, model = g/D.n_hyp, h = g - model*D.n_hyp;
    tv_fit(ws, model, D.xy1, D.xy2, D.norm1, D.norm2, D.subset + 8*h, lane, 64);
    if (lane < 9) D.hyp_model[9*(size_t)g + lane] = ws.model[lane];
}

__global__ __launch_bounds__(TV_T) void k_tv_score(TvDev D) {
    const int lane = threadIdx.x & 63, g = blockIdx.x*TV_NW + (threadIdx.x >> 6);
    if (g >= 2*D.n_hyp) return;                                             // (no barrier in this kernel)
    const int model = g/D.n_hyp;
    float m[9], hi[9] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
#pragma unroll
    for (int j = 0; j < 9; j++) m[j] = D.hyp_model[9*(size_t)g + j];
    if (model == 0) tv_h_inverse(m, hi);
    const float iss = tv_inv_sigma2(D.sigma);
    float s = 0.f;
#pragma unroll 1
    for (int base = 0; base < D.n; base += 64) {                            // the same trip count for every lane
        const int i = base + lane; float t1 = 0.f, t2 = 0.f;
        if (i < D.n) tv_terms(model, m, hi, D.xy1 + 2*(size_t)i, D.xy2 + 2*(size_t)i, iss, t1, t2);
        const int b1 = __float_as_int(t1), b2 = __float_as_int(t2);
#pragma unroll
        for (int k = 0; k < 64; k++) {                                      // a lane past n carries two zeros, which change no bit
            s = __fadd_rn(s, __int_as_float(__builtin_amdgcn_readlane(b1, k)));
            s = __fadd_rn(s, __int_as_float(__builtin_amdgcn_readlane(b2, k))); }
    }
    if (lane == 0) D.hyp_score[g] = s;
}

__global__ __launch_bounds__(TV_T) void k_tv_select(TvDev D) {
    __shared__ int s_sel[2];
    __shared__ float s_m[2][9], s_hi[9];
    __shared__ float s_sc[2*TSORB_TWOVIEW_MAX_HYP];
    const int tid = threadIdx.x;
    for (int j = tid; j < 2*D.n_hyp; j += TV_T) s_sc[j] = D.hyp_score[j];  // the scores once, side by side: the keep loops then read LDS, not 2 n_hyp dependent global loads
    __syncthreads();
    if (tid == 0 || tid == 64) { const int mdl = tid >> 6; float best;
        const int sel = tv_keep(s_sc + mdl*D.n_hyp, D.n_hyp, best);
        s_sel[mdl] = sel; D.sel[mdl] = sel; D.score[mdl] = best; }
    __syncthreads();
    if (tid < 18) { const int mdl = tid/9, j = tid - 9*mdl, sel = s_sel[mdl];
        const float v = sel >= 0 ? D.hyp_model[9*((size_t)mdl*D.n_hyp + sel) + j] : 0.f;
        s_m[mdl][j] = v; D.model[9*mdl + j] = v; }
    __syncthreads();
    if (tid == 0) tv_h_inverse(s_m[0], s_hi);
    __syncthreads();
    const float iss = tv_inv_sigma2(D.sigma); const bool have_h = s_sel[0] >= 0, have_f = s_sel[1] >= 0;
    for (int i = tid; i < D.n; i += TV_T) { float t1, t2; const float *p1 = D.xy1 + 2*(size_t)i, *p2 = D.xy2 + 2*(size_t)i;
        D.inl_h[i] = (have_h && tv_terms(0, s_m[0], s_hi, p1, p2, iss, t1, t2)) ? 1 : 0;
        D.inl_f[i] = (have_f && tv_terms(1, s_m[1], s_hi, p1, p2, iss, t1, t2)) ? 1 : 0; }
}
