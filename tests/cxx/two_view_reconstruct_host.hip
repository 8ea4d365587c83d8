// TEST / DIAGNOSTICS PROGRAM: the __host__ __device__ arithmetic of textslam_amd/csrc/tstwoview_rec.h on the CPU, one thread, no device call.
// Usage: two_view_reconstruct_host <in.bin> <out.bin> [reps]
//   in : int32 n, model, min_triangulated; float M21[9], K[4], sigma, min_parallax; float xy1[n][2], xy2[n][2]; uint8 inlier[n]
//   out: int32 result[6]; float R21[9], t21[3], p3d[n][3]; uint8 triangulated[n]; int32 hyp_good[8]; float hyp_cos[8], hyp_parallax[8], hyp_pose[8][12];
//        uint8 hyp_state[8][n]; float hyp_p3d[8][n][3]
//   reps > 0: additionally times `reps` runs of the whole reconstruction (hypotheses, every pair, the statistics, the keep logic) and prints "loop_ms <mean>".
// tests/test_two_view_reconstruct_ref.py builds it with the host sanitizers and compares it with the numpy restatement; tools/diag/gpu_two_view_reconstruct.py
// builds it with -O2 as the host baseline.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <chrono>
#include <vector>
#include "../../include/tsorb.h"
#include "../../textslam_amd/csrc/tstwoview_rec.h"

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "two_view_reconstruct_host: %s\n", msg); return 1; } while (0)
typedef std::chrono::steady_clock Clock;

int main(int argc, char **argv) {
    if (argc < 3) FAIL("usage: two_view_reconstruct_host in.bin out.bin [reps]");
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    int32_t n = 0, model = 0, min_tri = 0; float M[9], K[4], sigma = 0.f, min_par = 0.f;
    if (!rd(f, &n, 1) || !rd(f, &model, 1) || !rd(f, &min_tri, 1) || !rd(f, M, 9) || !rd(f, K, 4) || !rd(f, &sigma, 1) || !rd(f, &min_par, 1) ||
        n < 1 || n > TSORB_TWOVIEW_MAX_POINTS || model < 0 || model > 1 || min_tri < 0) FAIL("bad header");
    const size_t N = (size_t)n;
    std::vector<float> xy1(2*N), xy2(2*N); std::vector<uint8_t> inl(N);
    if (!rd(f, xy1.data(), xy1.size()) || !rd(f, xy2.data(), xy2.size()) || !rd(f, inl.data(), N)) FAIL("short input");
    fclose(f);
    const int H8 = TSORB_TWOVIEW_REC_HYP, nh = model == 0 ? 8 : 4;
    std::vector<float> p3d(3*N), hyp_p3d(3*N*H8), cosall(N*H8), hyp_pose(12*H8); std::vector<uint8_t> tri(N), state(N*H8);
    int32_t res[6], good[8]; float hcos[8], hpar[8], R21[9], t21[3]; uint32_t hist[256];
    int n_inl = 0; for (size_t i = 0; i < N; i++) n_inl += inl[i] != 0;
    double loop_ms = 0.0;
    for (int rep = 0; rep < (reps > 0 ? reps + 1 : 1); rep++) {             // run 0 is the one that is written (and the warm-up of the timed ones)
        const Clock::time_point t0 = Clock::now();
        std::fill(hyp_p3d.begin(), hyp_p3d.end(), 0.f); std::fill(state.begin(), state.end(), (uint8_t)0); std::fill(hyp_pose.begin(), hyp_pose.end(), 0.f);
        bool sv = false;
        for (int h = 0; h < nh && !sv; h++) { RecHyp hp; RecCam cam;
            sv = rec_form(model, M, K, h, hp, cam);
            if (sv) break;
            for (int j = 0; j < 12; j++) hyp_pose[12*(size_t)h + j] = j%4 < 3 ? hp.R[3*(j/4) + j%4] : hp.t[j/4];
            for (size_t i = 0; i < N; i++) { const size_t e = (size_t)h*N + i;
                state[e] = (uint8_t)rec_pair(hp, cam, K, rec_th2(sigma), inl[i] != 0, &xy1[2*i], &xy2[2*i], &hyp_p3d[3*e], cosall[e]); } }
        for (int h = 0; h < H8; h++) { good[h] = 0; hcos[h] = 0.f; hpar[h] = 0.f;
            if (h >= nh || sv) continue;
            const uint8_t *st = &state[(size_t)h*N];
            for (size_t i = 0; i < N; i++) good[h] += st[i] >= REC_ST_GOOD;
            if (good[h] > 0) { hcos[h] = rec_unkey(rec_select(st, &cosall[(size_t)h*N], n, good[h] - 1 < 50 ? good[h] - 1 : 50, hist, 0, 1)); hpar[h] = rec_parallax(hcos[h]); } }
        rec_keep(model, sv, good, hpar, n_inl, min_tri, min_par, res);
        const int sel = res[1];
        for (int j = 0; j < 9; j++) R21[j] = sel >= 0 ? hyp_pose[12*(size_t)sel + 4*(j/3) + j%3] : 0.f;
        for (int j = 0; j < 3; j++) t21[j] = sel >= 0 ? hyp_pose[12*(size_t)sel + 4*j + 3] : 0.f;
        for (size_t i = 0; i < N; i++) { const size_t e = (size_t)(sel >= 0 ? sel : 0)*N + i; const int st = sel >= 0 ? state[e] : REC_ST_OUT;
            for (int k = 0; k < 3; k++) p3d[3*i + k] = st >= REC_ST_GOOD ? hyp_p3d[3*e + k] : 0.f;
            tri[i] = st == REC_ST_TRI ? 1 : 0; }
        const Clock::time_point t1 = Clock::now();
        if (rep > 0) loop_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        else { FILE *o = fopen(argv[2], "wb"); if (!o) FAIL("cannot open output");
            wr(o, res, 6); wr(o, R21, 9); wr(o, t21, 3); wr(o, p3d.data(), p3d.size()); wr(o, tri.data(), N); wr(o, good, 8); wr(o, hcos, 8); wr(o, hpar, 8);
            wr(o, hyp_pose.data(), hyp_pose.size()); wr(o, state.data(), state.size()); wr(o, hyp_p3d.data(), hyp_p3d.size());
            fclose(o); }
    }
    if (reps > 0) printf("loop_ms %.6f (ok %d sel %d)\n", loop_ms/reps, res[0], res[1]);
    printf("two view reconstruct host: ok\n");
    return 0;
}
