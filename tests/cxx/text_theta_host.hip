// TEST / DIAGNOSTICS PROGRAM: the __host__ __device__ arithmetic of textslam_amd/csrc/tstexttheta.h on the CPU, one thread, no device call.
// Usage: text_theta_host <in.bin> <out.bin> [reps]
//   in : int32 n_plane, has_rho; int32 off[n_plane+1], hyp_off[n_plane+1]; double Tcr[12], K[4]; float host_xy[N][2], targ_xy[N][2]; double rho[N] if has_rho;
//        int32 triple[H][3]
//   out: int32 sel[n_plane]; double theta[n_plane][3], score[n_plane]; float p3d[N][3]; double rho[N], hyp_score[H], hyp_theta[H][3]
//   reps > 0: additionally times `reps` runs of the reference's loop (every feature triangulated, every hypothesis solved and scored, the keep loop) and prints
//   "loop_ms <mean>".
// tests/test_text_theta_ref.py builds it with the host sanitizers and compares it with the numpy restatement; tools/diag/gpu_text_theta.py builds it with -O2 as the
// host baseline.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <chrono>
#include <vector>
#include "../../include/tsorb.h"
#include "../../textslam_amd/csrc/tstexttheta.h"

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "text_theta_host: %s\n", msg); return 1; } while (0)
typedef std::chrono::steady_clock Clock;

int main(int argc, char **argv) {
    if (argc < 3) FAIL("usage: text_theta_host in.bin out.bin [reps]");
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    int32_t P = 0, has_rho = 0;
    if (!rd(f, &P, 1) || !rd(f, &has_rho, 1) || P < 0 || P > (1 << 20)) FAIL("bad header");
    std::vector<int32_t> off((size_t)P + 1), hoff((size_t)P + 1); double T[12], K[4];
    if (!rd(f, off.data(), off.size()) || !rd(f, hoff.data(), hoff.size()) || !rd(f, T, 12) || !rd(f, K, 4) || off[0] != 0 || hoff[0] != 0) FAIL("bad offsets");
    for (int p = 0; p < P; p++) if (off[p + 1] < off[p] || off[p + 1] - off[p] > TSORB_THETA_MAX_FEAT || hoff[p + 1] < hoff[p]) FAIL("bad plane");
    const size_t N = (size_t)off[P], H = (size_t)hoff[P];
    std::vector<float> hxy(2*N), txy(2*N); std::vector<double> rho_in(has_rho ? N : 0); std::vector<int32_t> tri(3*H);
    if (!rd(f, hxy.data(), hxy.size()) || !rd(f, txy.data(), txy.size()) || !rd(f, rho_in.data(), rho_in.size()) || !rd(f, tri.data(), tri.size())) FAIL("short input");
    fclose(f);
    for (int p = 0; p < P; p++) for (size_t e = 3*(size_t)hoff[p]; e < 3*(size_t)hoff[p + 1]; e++) if (tri[e] < 0 || tri[e] >= off[p + 1] - off[p]) FAIL("triple outside the plane");
    std::vector<int32_t> sel((size_t)P); std::vector<double> theta(3*(size_t)P), score((size_t)P), rho(N), hs(H), ht(3*H); std::vector<float> p3d(3*N);
    std::vector<double> F[5]; for (int k = 0; k < 5; k++) F[k].resize(TSORB_THETA_MAX_FEAT);
    double loop_ms = 0.0;
    for (int rep = 0; rep < (reps > 0 ? reps + 1 : 1); rep++) {             // run 0 is the one that is written (and the warm-up of the timed ones)
        const Clock::time_point t0 = Clock::now();
        for (size_t i = 0; i < N; i++) { float X[3] = { 0.f, 0.f, 0.f };
            if (has_rho) rho[i] = rho_in[i]; else tt_triangulate(T, K, &hxy[2*i], &txy[2*i], X, rho[i]);
            p3d[3*i] = X[0]; p3d[3*i + 1] = X[1]; p3d[3*i + 2] = X[2]; }
        for (int p = 0; p < P; p++) { const int a = off[p], n = off[p + 1] - a, h0 = hoff[p], nh = hoff[p + 1] - h0;
            for (int i = 0; i < n && n >= 3; i++) { double v[5]; tt_feature(K, &hxy[2*(size_t)(a + i)], &txy[2*(size_t)(a + i)], rho[(size_t)(a + i)], v);
                for (int k = 0; k < 5; k++) F[k][(size_t)i] = v[k]; }
            for (int h = 0; h < nh; h++) { const size_t e = (size_t)(h0 + h);
                if (n < 3) { hs[e] = 0.0; ht[3*e] = 0.0; ht[3*e + 1] = 0.0; ht[3*e + 2] = 0.0; continue; }
                hs[e] = tt_hypothesis(T, K, n, F[0].data(), F[1].data(), F[2].data(), F[3].data(), F[4].data(), &tri[3*e], &ht[3*e]); }
            double best = -1.0; int idx = -1;
            if (n >= 3 && nh > 0) tt_scan(&hs[(size_t)h0], nh, 0, 1, best, idx);
            if (n >= 3 && nh > 0) {                                         // the device's way to the same answer: 64 lanes' scans, then the butterfly
                double b64[64]; int i64[64];
                for (int l = 0; l < 64; l++) tt_scan(&hs[(size_t)h0], nh, l, 64, b64[l], i64[l]);
                for (int m = 32; m > 0; m >>= 1) { double nb[64]; int ni[64];
                    for (int l = 0; l < 64; l++) { const bool t = tt_takes(b64[l], i64[l], b64[l ^ m], i64[l ^ m]); nb[l] = t ? b64[l ^ m] : b64[l]; ni[l] = t ? i64[l ^ m] : i64[l]; }
                    for (int l = 0; l < 64; l++) { b64[l] = nb[l]; i64[l] = ni[l]; } }
                if (i64[0] != idx || (idx >= 0 && b64[0] != best)) FAIL("the lanes' selection differs from the reference's loop"); }
            sel[(size_t)p] = idx; score[(size_t)p] = idx >= 0 ? best : 0.0;
            for (int k = 0; k < 3; k++) theta[3*(size_t)p + k] = idx >= 0 ? ht[3*(size_t)(h0 + idx) + k] : 0.0; }
        const Clock::time_point t1 = Clock::now();
        if (rep > 0) loop_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        else { FILE *o = fopen(argv[2], "wb"); if (!o) FAIL("cannot open output");
            wr(o, sel.data(), sel.size()); wr(o, theta.data(), theta.size()); wr(o, score.data(), score.size()); wr(o, p3d.data(), p3d.size()); wr(o, rho.data(), rho.size());
            wr(o, hs.data(), hs.size()); wr(o, ht.data(), ht.size());
            fclose(o); }
    }
    if (reps > 0) printf("loop_ms %.6f (planes %d)\n", loop_ms/reps, (int)P);
    printf("text theta host: ok\n");
    return 0;
}
