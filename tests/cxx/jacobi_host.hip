// TEST PROGRAM: the __host__ __device__ small-matrix iterations of textslam_amd/csrc/tsjacobi.h on the CPU, one thread, no device call.  It includes that header alone.
// Usage: jacobi_host <in.bin> <out.bin>
//   in : int32 n_rec; per record int32 kind, int32 N (3 or 4), double a[N][N]
//   out: per record, by kind
//        0  one-sided, the callers' thresholds (JAC_ORTHO, JAC_TINY): double G[N][N], Q[N][N]; int32 jmin (jac_shortest)
//        1  two-sided on the symmetric a, sweeps of jac_sym_rotate until the off-diagonal sum is not above zero -- the loop and pair order of pnp_sym3_eig (N = 3: 01 02 12,
//           at most 40 sweeps) and of horn_sim3 (N = 4: 01 02 03 12 13 23, at most 24): double A[N][N], V[N][N]; int32 sweeps
//        2  one-sided with pnp_polar3's thresholds (1e-17, no second test), N = 3 only: as kind 0
//        3  jac_null4 (N = 4 only): double v[4]
//        4  the sign rule on the rows of a: int32 jac_negative(row, N) per row, then (N = 3 only) int32 jac_negative3 per row
//   then the round-robin order: for M = 9 (pairs i = 0 .. 4, i = 0 the bye's) and M = 11 (i = 0 .. 5), for r = 0 .. M - 1, for i: int32 p, q
// tests/test_jacobi_host.py builds it with the host sanitizers and checks properties of what it returns with numpy.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <vector>
#include "../../textslam_amd/csrc/tsjacobi.h"

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "jacobi_host: %s\n", msg); return 1; } while (0)

template <int N> static void one_sided(const double *a, double ortho, double tiny, FILE *o) {
    double G[N][N], Q[N][N];
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) G[i][j] = a[N*i + j];
    jac_orthogonalize(G, Q, ortho, tiny);
    const int32_t jmin = jac_shortest(G);
    wr(o, &G[0][0], N*N); wr(o, &Q[0][0], N*N); wr(o, &jmin, 1);
}

template <int N> static void two_sided(const double *a, FILE *o) {
    double A[N][N], V[N][N];
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) { A[i][j] = a[N*i + j]; V[i][j] = i == j ? 1.0 : 0.0; }
    int32_t sweeps = 0;
    if constexpr (N == 3) {
        for (; sweeps < 40; sweeps++) {
            if (!(fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]) > 0.0)) break;
            jac_sym_rotate<3, 0, 1>(A, V); jac_sym_rotate<3, 0, 2>(A, V); jac_sym_rotate<3, 1, 2>(A, V); }
    } else {
        for (; sweeps < 24; sweeps++) {
            if (!(fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]) > 0.0)) break;
            jac_sym_rotate<4, 0, 1>(A, V); jac_sym_rotate<4, 0, 2>(A, V); jac_sym_rotate<4, 0, 3>(A, V);
            jac_sym_rotate<4, 1, 2>(A, V); jac_sym_rotate<4, 1, 3>(A, V); jac_sym_rotate<4, 2, 3>(A, V); }
    }
    wr(o, &A[0][0], N*N); wr(o, &V[0][0], N*N); wr(o, &sweeps, 1);
}

template <int M> static void schedule(FILE *o) {
    for (int r = 0; r < M; r++) for (int i = 0; i <= M/2; i++) { int p, q; jac_pair<M>(r, i, p, q); const int32_t pq[2] = { p, q }; wr(o, pq, 2); }
}

int main(int argc, char **argv) {
    if (argc < 3) FAIL("usage: jacobi_host in.bin out.bin");
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    FILE *o = fopen(argv[2], "wb"); if (!o) FAIL("cannot open output");
    int32_t n_rec = 0;
    if (!rd(f, &n_rec, 1) || n_rec < 0) FAIL("bad header");
    for (int k = 0; k < n_rec; k++) {
        int32_t hd[2]; double a[16];
        if (!rd(f, hd, 2) || (hd[1] != 3 && hd[1] != 4) || !rd(f, a, (size_t)(hd[1]*hd[1]))) FAIL("bad record");
        const int kind = hd[0], N = hd[1];
        if (kind == 0) { if (N == 3) one_sided<3>(a, JAC_ORTHO, JAC_TINY, o); else one_sided<4>(a, JAC_ORTHO, JAC_TINY, o); }
        else if (kind == 1) { if (N == 3) two_sided<3>(a, o); else two_sided<4>(a, o); }
        else if (kind == 2 && N == 3) one_sided<3>(a, 1e-17, 0.0, o);
        else if (kind == 3 && N == 4) { double G[4][4], v[4];
            for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) G[i][j] = a[4*i + j];
            jac_null4(G, v); wr(o, v, 4); }
        else if (kind == 4) {
            for (int i = 0; i < N; i++) { const int32_t neg = jac_negative(a + N*i, N) ? 1 : 0; wr(o, &neg, 1); }
            if (N == 3) for (int i = 0; i < 3; i++) { const int32_t neg = jac_negative3(a[3*i], a[3*i + 1], a[3*i + 2]) ? 1 : 0; wr(o, &neg, 1); } }
        else FAIL("bad kind");
    }
    fclose(f);
    schedule<9>(o); schedule<11>(o);
    fclose(o);
    printf("jacobi host: ok\n");
    return 0;
}
