// TEST / DIAGNOSTICS PROGRAM: the __host__ __device__ arithmetic of textslam_amd/csrc/tstwoview.h on the CPU, one thread, no device call.
// Usage: two_view_host <in.bin> <out.bin> [reps]
//   in : int32 n, int32 H, float norm1[4], float norm2[4], float sigma, float xy1[n][2], float xy2[n][2], int32 subset[H][8]
//   out: float hyp_model[2][H][9], float hyp_score[2][H], int32 sel[2], float score[2], float H21[9], float F21[9], uint8 inlier_h[n], uint8 inlier_f[n]
//   reps > 0: additionally times `reps` runs of FindHomography's + FindFundamental's loops (2 H fits, 2 H scorings over all matches, the keep loops; the reference
//             has no early stop) and prints "loop_ms <mean> fit_ms <mean> score_ms <mean>".
//   Always prints the Jacobi sweeps the fits took ("sweeps: H mean .. most .., F mean .. most ..").
// tests/test_two_view_ref.py builds it with the host sanitizers and compares it with the numpy restatement; tools/diag/gpu_two_view.py builds it with -O2 as the
// host baseline.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <chrono>
#include <vector>
#include "../../include/tsorb.h"
#include "../../textslam_amd/csrc/tstwoview.h"

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "two_view_host: %s\n", msg); return 1; } while (0)
typedef std::chrono::steady_clock Clock;

int main(int argc, char **argv) {
    if (argc < 3) FAIL("usage: two_view_host in.bin out.bin [reps]");
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    int32_t n = 0, H = 0; float n1[4], n2[4], sigma = 0.f;
    if (!rd(f, &n, 1) || !rd(f, &H, 1) || !rd(f, n1, 4) || !rd(f, n2, 4) || !rd(f, &sigma, 1) || n < 8 || n > TSORB_TWOVIEW_MAX_POINTS || H < 1 || H > TSORB_TWOVIEW_MAX_HYP)
        FAIL("bad header");
    std::vector<float> xy1(2*(size_t)n), xy2(2*(size_t)n); std::vector<int32_t> subset(8*(size_t)H);
    if (!rd(f, xy1.data(), xy1.size()) || !rd(f, xy2.data(), xy2.size()) || !rd(f, subset.data(), subset.size())) FAIL("short input");
    fclose(f);
    for (size_t i = 0; i < subset.size(); i++) if (subset[i] < 0 || subset[i] >= n) FAIL("subset index outside [0, n)");
    std::vector<float> hyp_model(18*(size_t)H), hyp_score(2*(size_t)H); std::vector<uint8_t> inl_h((size_t)n, 0), inl_f((size_t)n, 0);
    int32_t sel[2]; float score[2], kept[18];
    TvWs *W = new TvWs;
    double fit_ms = 0.0, score_ms = 0.0, loop_ms = 0.0; long sweeps[2] = { 0, 0 }; int most[2] = { 0, 0 };
    for (int rep = 0; rep < (reps > 0 ? reps + 1 : 1); rep++) {             // run 0 is the one that is written (and the warm-up of the timed ones)
        const Clock::time_point t0 = Clock::now();
        for (int g = 0; g < 2*H; g++) { const int model = g/H, h = g - model*H;
            tv_fit(*W, model, xy1.data(), xy2.data(), n1, n2, subset.data() + 8*h, 0, 1);
            if (rep == 0) { sweeps[model] += W->sweeps; if (W->sweeps > most[model]) most[model] = W->sweeps; }
            for (int j = 0; j < 9; j++) hyp_model[9*(size_t)g + j] = W->model[j]; }
        const Clock::time_point t1 = Clock::now();
        for (int g = 0; g < 2*H; g++) hyp_score[(size_t)g] = tv_score_serial(g/H, &hyp_model[9*(size_t)g], n, xy1.data(), xy2.data(), sigma, 0);
        for (int m = 0; m < 2; m++) { sel[m] = tv_keep(&hyp_score[(size_t)m*H], H, score[m]);
            for (int j = 0; j < 9; j++) kept[9*m + j] = sel[m] >= 0 ? hyp_model[9*((size_t)m*H + sel[m]) + j] : 0.f;
            uint8_t *mask = m == 0 ? inl_h.data() : inl_f.data();
            if (sel[m] >= 0) tv_score_serial(m, kept + 9*m, n, xy1.data(), xy2.data(), sigma, mask); else for (int i = 0; i < n; i++) mask[i] = 0; }
        const Clock::time_point t2 = Clock::now();
        if (rep > 0) { fit_ms += std::chrono::duration<double, std::milli>(t1 - t0).count(); score_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
            loop_ms += std::chrono::duration<double, std::milli>(t2 - t0).count(); }
        else { FILE *o = fopen(argv[2], "wb"); if (!o) FAIL("cannot open output");
            wr(o, hyp_model.data(), hyp_model.size()); wr(o, hyp_score.data(), hyp_score.size()); wr(o, sel, 2); wr(o, score, 2); wr(o, kept, 18);
            wr(o, inl_h.data(), inl_h.size()); wr(o, inl_f.data(), inl_f.size());
            fclose(o); }
    }
    if (reps > 0) printf("loop_ms %.6f fit_ms %.6f score_ms %.6f (sel %d %d)\n", loop_ms/reps, fit_ms/reps, score_ms/reps, sel[0], sel[1]);
    printf("sweeps: H mean %.2f most %d, F mean %.2f most %d\n", (double)sweeps[0]/H, most[0], (double)sweeps[1]/H, most[1]);
    delete W;
    printf("two view host: ok\n");
    return 0;
}
