// TEST / DIAGNOSTICS PROGRAM: the __host__ __device__ arithmetic of textslam_amd/csrc/tspnp.h on the CPU, one thread, no device call.
// Usage: pnp_host <in.bin> <out.bin> [reps]
//   in : int32 n, int32 H, double K[4], double reproj_err, double confidence, float Pw[n][3], float uv[n][2], int32 subset[H][5]
//   out: double hyp_pose[H][12], int32 hyp_count[H], int32 result[4], uint8 inlier[n]        (every hypothesis evaluated, as the library does)
//   reps > 0: additionally times `reps` runs of the reference's loop WITH its early stop (a hypothesis is formed and counted only when the loop reaches it)
//             and prints "early_stop_ms <mean> n_run <k>".
// tests/test_pnp_ransac_ref.py builds it with the host sanitizers and compares its poses with the numpy restatement; tools/diag/gpu_pnp_ransac.py builds it with -O2 as
// the host baseline.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <chrono>
#include <vector>
#include "../../include/tsorb.h"
#include "../../textslam_amd/csrc/tspnp.h"

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "pnp_host: %s\n", msg); return 1; } while (0)

static int count_of(const double *pose, const double K[4], int n, const float *Pw, const float *uv, float thr) {
    int c = 0;
    for (int i = 0; i < n; i++) c += pnp_inlier(pose, K, Pw + 3*i, uv + 2*i, thr) ? 1 : 0;
    return c;
}

int main(int argc, char **argv) {
    if (argc < 3) FAIL("usage: pnp_host in.bin out.bin [reps]");
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    int32_t n = 0, H = 0; double K[4], reproj = 0.0, conf = 0.0;
    if (!rd(f, &n, 1) || !rd(f, &H, 1) || !rd(f, K, 4) || !rd(f, &reproj, 1) || !rd(f, &conf, 1) || n < 5 || H < 1 || H > TSORB_PNP_MAX_HYP) FAIL("bad header");
    std::vector<float> Pw(3*(size_t)n), uv(2*(size_t)n); std::vector<int32_t> subset(5*(size_t)H);
    if (!rd(f, Pw.data(), Pw.size()) || !rd(f, uv.data(), uv.size()) || !rd(f, subset.data(), subset.size())) FAIL("short input");
    fclose(f);
    for (size_t i = 0; i < subset.size(); i++) if (subset[i] < 0 || subset[i] >= n) FAIL("subset index outside [0, n)");
    const float thr = (float)(reproj*reproj);
    std::vector<double> hyp_pose(12*(size_t)H); std::vector<int32_t> count((size_t)H); std::vector<uint8_t> inlier((size_t)n, 0); int32_t result[4];
    PnpWs *W = new PnpWs;
    for (int h = 0; h < H; h++) {
        pnp_hypothesis(*W, Pw.data(), uv.data(), subset.data() + 5*h, K, 0, 1);
        for (int j = 0; j < 12; j++) hyp_pose[12*(size_t)h + j] = W->pose[j];
        count[(size_t)h] = count_of(W->pose, K, n, Pw.data(), uv.data(), thr);
    }
    pnp_walk(count.data(), H, n, conf, result);
    if (result[0]) for (int i = 0; i < n; i++) inlier[(size_t)i] = pnp_inlier(&hyp_pose[12*(size_t)result[2]], K, &Pw[3*(size_t)i], &uv[2*(size_t)i], thr) ? 1 : 0;
    FILE *g = fopen(argv[2], "wb"); if (!g) FAIL("cannot open output");
    wr(g, hyp_pose.data(), hyp_pose.size()); wr(g, count.data(), count.size()); wr(g, result, 4); wr(g, inlier.data(), inlier.size());
    fclose(g);
    if (reps > 0) {
        int n_run = 0, keep = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; r++) {                                    // RANSACPointSetRegistrator::run's loop, the hypothesis formed when the loop reaches it
            int max_good = 0, niters = H, iter = 0;
            for (; iter < niters; iter++) {
                pnp_hypothesis(*W, Pw.data(), uv.data(), subset.data() + 5*iter, K, 0, 1);
                const int c = count_of(W->pose, K, n, Pw.data(), uv.data(), thr);
                if (c > (max_good > 4 ? max_good : 4)) { max_good = c; niters = pnp_update_iters(conf, (double)(n - c)/n, niters); }
            }
            n_run = iter; keep += max_good;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()/reps;
        printf("early_stop_ms %.6f n_run %d (checksum %d)\n", ms, n_run, keep);
    }
    delete W;
    printf("pnp host: ok\n");
    return 0;
}
