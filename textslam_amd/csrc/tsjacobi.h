// tsjacobi.h -- the small fp64 Jacobi iterations of the front-end and of loop closing, once each: the one-sided (Hestenes) iteration that turns the columns of a 3 x 3 or
// 4 x 4 until they are orthogonal, the two-sided (Rutishauser) rotation of a symmetric matrix, the round-robin order of the parallel iterations, the sign rule of a
// singular vector -- and the seam between a kernel and the host program that runs the same arithmetic.  tspnp.h, tstwoview.h, tstwoview_rec.h, tstexttheta.h (libtsorb)
// and tsloop_ransac.h (libtsloop) include it.  Everything is __host__ __device__; no kernel, no struct of any call.  The matrices are arrays with compile-time sizes and
// pair indices: after inlining they are registers on the device.  Every loop is bounded.
#pragma once
#pragma clang fp contract(off)

// ---- the host / device seam: a host program calls the per-item arithmetic with (lane, lane count) = (0, 1) and runs what the kernel runs
#ifdef __HIP_DEVICE_COMPILE__
#define TS_BARRIER() __syncthreads()
#define TS_ALL(x) __syncthreads_and(x)         // the barrier with a vote: true when x holds on every thread of the workgroup
#define TS_COUNT(x) atomicAdd(&(x), 1u)
#define TS_FMUL(a, b) __fmul_rn(a, b)          // float arithmetic whose bits matter: one rounding each, no contraction
#define TS_FADD(a, b) __fadd_rn(a, b)
#define TS_FSUB(a, b) __fsub_rn(a, b)
#define TS_FDIV(a, b) __fdiv_rn(a, b)
#else
#define TS_BARRIER() do { } while (0)
#define TS_ALL(x) (x)
#define TS_COUNT(x) ((x)++)
#define TS_FMUL(a, b) ((float)(a)*(float)(b))
#define TS_FADD(a, b) ((float)(a) + (float)(b))
#define TS_FSUB(a, b) ((float)(a) - (float)(b))
#define TS_FDIV(a, b) ((float)(a)/(float)(b))
#endif

__host__ __device__ __forceinline__ double ts_nan() { return __builtin_nan(""); }

#define JAC_SWEEPS 40             // three or four columns are orthogonal after 4 - 8 sweeps; the bound only has to be finite
#define JAC_ORTHO 1e-14           // |a_p . a_q| <= JAC_ORTHO |a_p| |a_q|: the pair counts as orthogonal
#define JAC_TINY 1e-17            // ... and so does one whose rotation angle (below |a_p . a_q| / (|a_p|^2 + |a_q|^2)) could not change a double of the rotations

// ---- the sign rule of a vector known up to sign: the component of largest magnitude is positive, the first on ties.  True when v has to be negated for that
__host__ __device__ __forceinline__ bool jac_negative(const double *v, int n) {
    int k = 0;
    for (int i = 1; i < n; i++) if (fabs(v[i]) > fabs(v[k])) k = i;
    return v[k] < 0.0;
}
__host__ __device__ __forceinline__ bool jac_negative3(double a, double b, double c) { const double v[3] = { a, b, c }; return jac_negative(v, 3); }
__host__ __device__ __forceinline__ void jac_sign(double *v, int n) {
    if (jac_negative(v, n)) for (int i = 0; i < n; i++) v[i] = -v[i];
}

// ---- the round-robin (circle method) order over an odd modulus M: pair i of step r (0 .. M - 1), p < q.  Over M indices and a bye the pairs of a step are i = 1 ..
// (M - 1)/2 and i = 0 would be the bye's; over M + 1 indices pair 0 is (r, M): index M stays, the others turn.  A sweep of M steps holds every pair once
template <int M>
__host__ __device__ __forceinline__ void jac_pair(int r, int i, int &p, int &q) {
    const int a = i == 0 ? M : (r + i)%M, b = (r + M - i)%M;
    p = a < b ? a : b; q = a < b ? b : a;
}

// ---- one-sided: G = A Q, the columns of G turned in pairs until they are orthogonal; then |G_j| are A's singular values and the columns of Q its right singular vectors
// the rotation that makes two columns with squared lengths al, be and product ga orthogonal; false (c = 1, s = 0) when they count as orthogonal already: ga is at most
// ortho sqrt(al be) or at most tiny (al + be), or a NaN is among them (a NaN never turns).  tiny = 0.0 is no second test: |ga| > 0 (al + be) fails only where the first
// test does (al + be overflows only where al be does; al + be = NaN makes al be NaN)
__host__ __device__ __forceinline__ bool jac_rotation(double al, double be, double ga, double ortho, double tiny, double &c, double &s) {
    c = 1.0; s = 0.0;
    if (!(fabs(ga) > ortho*sqrt(al*be)) || !(fabs(ga) > tiny*(al + be))) return false;
    const double zeta = (be - al)/(2.0*ga);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0)/(fabs(zeta) + sqrt(zeta*zeta + 1.0));
    c = 1.0/sqrt(t*t + 1.0); s = t*c;
    return true;
}

// one step on the columns (p, q) of G, Q <- Q J: returns whether it turned them
template <int N, int p, int q>
__host__ __device__ __forceinline__ bool jac_turn(double G[N][N], double Q[N][N], double ortho, double tiny) {
    double al = 0.0, be = 0.0, ga = 0.0, c, s;
#pragma unroll
    for (int i = 0; i < N; i++) { al += G[i][p]*G[i][p]; be += G[i][q]*G[i][q]; ga += G[i][p]*G[i][q]; }
    if (!jac_rotation(al, be, ga, ortho, tiny, c, s)) return false;
#pragma unroll
    for (int i = 0; i < N; i++) { const double gp = G[i][p], gq = G[i][q]; G[i][p] = c*gp - s*gq; G[i][q] = s*gp + c*gq; }
#pragma unroll
    for (int i = 0; i < N; i++) { const double vp = Q[i][p], vq = Q[i][q]; Q[i][p] = c*vp - s*vq; Q[i][q] = s*vp + c*vq; }
    return true;
}

// Q = I, then sweeps over the pairs (3 x 3: 01 02 12; 4 x 4: 01 23 02 13 03 12) until one turns nothing: the caller's own matrix, so a lane stops when ITS matrix has
// converged.  (Q = I is a copy of a constant, not nine stores: written as stores it costs k_tv_fit 18 VGPRs and an occupancy class)
__host__ __device__ inline void jac_orthogonalize(double G[3][3], double Q[3][3], double ortho, double tiny) {
    const double I[3][3] = { {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0} };
    __builtin_memcpy(Q, I, sizeof I);
#pragma unroll 1
    for (int sweep = 0; sweep < JAC_SWEEPS; sweep++) {
        const bool a = jac_turn<3, 0, 1>(G, Q, ortho, tiny), b = jac_turn<3, 0, 2>(G, Q, ortho, tiny), c = jac_turn<3, 1, 2>(G, Q, ortho, tiny);
        if (!(a || b || c)) break; }
}
__host__ __device__ inline void jac_orthogonalize(double G[4][4], double Q[4][4], double ortho, double tiny) {
    const double I[4][4] = { {1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0} };
    __builtin_memcpy(Q, I, sizeof I);
#pragma unroll 1
    for (int sweep = 0; sweep < JAC_SWEEPS; sweep++) {
        const bool a = jac_turn<4, 0, 1>(G, Q, ortho, tiny), b = jac_turn<4, 2, 3>(G, Q, ortho, tiny), c = jac_turn<4, 0, 2>(G, Q, ortho, tiny),
                   d = jac_turn<4, 1, 3>(G, Q, ortho, tiny), e = jac_turn<4, 0, 3>(G, Q, ortho, tiny), f = jac_turn<4, 1, 2>(G, Q, ortho, tiny);
        if (!(a || b || c || d || e || f)) break; }
}

// the squared length of column j, and the shortest column (the smallest singular value), the first of equal ones
__host__ __device__ __forceinline__ double jac_length2(const double G[3][3], int j) { return (G[0][j]*G[0][j] + G[1][j]*G[1][j]) + G[2][j]*G[2][j]; }
__host__ __device__ __forceinline__ double jac_length2(const double G[4][4], int j) { return ((G[0][j]*G[0][j] + G[1][j]*G[1][j]) + G[2][j]*G[2][j]) + G[3][j]*G[3][j]; }
__host__ __device__ __forceinline__ int jac_shortest(const double G[3][3]) {
    const double d[3] = { jac_length2(G, 0), jac_length2(G, 1), jac_length2(G, 2) };
    return d[1] < d[0] ? (d[2] < d[1] ? 2 : 1) : (d[2] < d[0] ? 2 : 0);
}
__host__ __device__ __forceinline__ int jac_shortest(const double G[4][4]) {
    const double d[4] = { jac_length2(G, 0), jac_length2(G, 1), jac_length2(G, 2), jac_length2(G, 3) };
    const int j01 = d[1] < d[0] ? 1 : 0, j23 = d[3] < d[2] ? 3 : 2; const double m01 = j01 ? d[1] : d[0], m23 = j23 == 3 ? d[3] : d[2];
    return m23 < m01 ? j23 : j01;
}
// entry i of column j of a 4 x 4 for a j known only at run time: selects, not an indexed (private-memory) read
__host__ __device__ __forceinline__ double jac_entry(const double Q[4][4], int i, int j) { return j == 0 ? Q[i][0] : j == 1 ? Q[i][1] : j == 2 ? Q[i][2] : Q[i][3]; }

// the right singular vector of the smallest singular value of the 4 x 4 in G (the first of equal ones), up to sign and of unit length up to rounding: G is turned in place
__host__ __device__ __forceinline__ void jac_null4(double G[4][4], double v[4]) {
    double Q[4][4];
    jac_orthogonalize(G, Q, JAC_ORTHO, JAC_TINY);
    const int jmin = jac_shortest(G);
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = jac_entry(Q, i, jmin);
}

// ---- two-sided: A <- J^T A J on a symmetric A, V <- V J; then the diagonal of A holds the eigenvalues and the columns of V the eigenvectors
// the rotation that annihilates a_pq (Rutishauser); false (c = 1, s = 0) when there is nothing to rotate: a_pq is zero, or negligible beside both diagonals -- then the
// caller sets it to zero
__host__ __device__ __forceinline__ bool jac_sym_rotation(double app, double aqq, double apq, double &c, double &s) {
    c = 1.0; s = 0.0;
    if (apq == 0.0) return false;
    const double g = 100.0*fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) return false;
    const double theta = (aqq - app)/(2.0*apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0)/(fabs(theta) + sqrt(theta*theta + 1.0));
    c = 1.0/sqrt(t*t + 1.0); s = t*c;
    return true;
}

// one rotation of the pair (p, q).  Nothing to rotate: a zero a_pq is left as it is (its sign included), a negligible one becomes zero, nothing else is touched
template <int N, int p, int q>
__host__ __device__ __forceinline__ void jac_sym_rotate(double A[N][N], double V[N][N]) {
    double c, s;
    if (!jac_sym_rotation(A[p][p], A[q][q], A[p][q], c, s)) { if (A[p][q] != 0.0) { A[p][q] = 0.0; A[q][p] = 0.0; } return; }
#pragma unroll
    for (int k = 0; k < N; k++) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c*akp - s*akq; A[k][q] = s*akp + c*akq; }
#pragma unroll
    for (int k = 0; k < N; k++) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c*apk - s*aqk; A[q][k] = s*apk + c*aqk; }
    A[p][q] = 0.0; A[q][p] = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c*vkp - s*vkq; V[k][q] = s*vkp + c*vkq; }
}
