// TEST DRIVER: loopClosing::ComputeSim3's step 3 from C++ -- adapter/tsloop_sim3_ransac.hpp over the mock types of mock_textslam.hpp, one
// tsloop_sim3_batch call for all candidates.  Usage: sim3_ransac_from_cxx <in.bin> <out.bin>
//   in : int32 n_cand, uint32 seed, double K1[4], double K[4]; per candidate: int32 n, double K2[4], P1[n][3], P2[n][3], pred1[n][2], pred2[n][2] (double),
//        uv1[n][2], uv2[n][2] (float)
//   out: per candidate: int32 H, triple[H][3], int32 ok, sel, n_inlier_ransac, nInliersOpt (-1: discarded), double sim_ransac[8], sim[8],
//        int32 iters, accepted, termination, n_inlier, double cost0, cost1, uint8 inlier[n], int32 hyp_count[H], double hyp_sim[H][8]
// tests/test_gpu_sim3_ransac.py predicts the triples with the same generator restated in Python and holds the outputs equal to the Python mirror's.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mock_textslam.hpp"
#include "tsloop_sim3_ransac.hpp"

struct KeyFrame : mock::keyframe { mock::Mat33 mK; };                 // keyframe::mK: the 3 x 3 intrinsics

// a 32-bit linear congruential generator written for this driver (Numerical Recipes' constants), standing where DUtils::Random::RandomInt stands
static uint32_t g_lcg = 0;
struct Traits : mock::Traits {
    static int random_int(int lo, int hi) { g_lcg = g_lcg*1664525u + 1013904223u; return lo + (int)((g_lcg >> 8) % (uint32_t)(hi - lo + 1)); }
};

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "sim3_ransac_from_cxx: %s\n", msg); return 1; } while (0)

int main(int argc, char **argv) {
    if (argc != 3) FAIL("usage: sim3_ransac_from_cxx in.bin out.bin");
    {   // the hypothesis-count rule: SetRansacParameters(0.99, 20, 300), iterate(5, ...)
        const int N[] = { 0, 19, 20, 21, 22, 24, 25, 60, 300, 1500 }, H[] = { 0, 0, 1, 3, 4, 5, 5, 5, 5, 5 };
        for (int i = 0; i < 10; i++) if (tsloop_adapter::sim3_num_hypotheses(N[i]) != H[i]) FAIL("sim3_num_hypotheses");
    }
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    int32_t nc = 0; uint32_t seed = 0; double K1[4], K[4];
    if (!rd(f, &nc, 1) || !rd(f, &seed, 1) || !rd(f, K1, 4) || !rd(f, K, 4) || nc < 0) FAIL("short input");
    KeyFrame cur; cur.mK = mock::Mat33(); for (int i = 0; i < 9; i++) cur.mK.m[i] = 0.0;
    cur.mK(0, 0) = K1[0]; cur.mK(1, 1) = K1[1]; cur.mK(0, 2) = K1[2]; cur.mK(1, 2) = K1[3]; cur.mK(2, 2) = 1.0;
    std::vector<KeyFrame> kfs((size_t)nc); std::vector<KeyFrame *> vKFCands;
    std::vector<std::vector<mock::FeatureConvert> > vvCur((size_t)nc), vvCan((size_t)nc);
    for (int k = 0; k < nc; k++) {
        int32_t n = 0; double K2[4];
        if (!rd(f, &n, 1) || !rd(f, K2, 4) || n < 0) FAIL("short input");
        for (int i = 0; i < 9; i++) kfs[(size_t)k].mK.m[i] = 0.0;
        kfs[(size_t)k].mK(0, 0) = K2[0]; kfs[(size_t)k].mK(1, 1) = K2[1]; kfs[(size_t)k].mK(0, 2) = K2[2]; kfs[(size_t)k].mK(1, 2) = K2[3]; kfs[(size_t)k].mK(2, 2) = 1.0;
        vKFCands.push_back(&kfs[(size_t)k]);
        std::vector<double> P1(3*(size_t)n), P2(3*(size_t)n), q1(2*(size_t)n), q2(2*(size_t)n); std::vector<float> u1(2*(size_t)n), u2(2*(size_t)n);
        if (!rd(f, P1.data(), P1.size()) || !rd(f, P2.data(), P2.size()) || !rd(f, q1.data(), q1.size()) || !rd(f, q2.data(), q2.size()) ||
            !rd(f, u1.data(), u1.size()) || !rd(f, u2.data(), u2.size())) FAIL("short input");
        vvCur[(size_t)k].resize((size_t)n); vvCan[(size_t)k].resize((size_t)n);
        for (size_t i = 0; i < (size_t)n; i++) {
            mock::FeatureConvert &a = vvCur[(size_t)k][i], &b = vvCan[(size_t)k][i];
            for (int c = 0; c < 3; c++) { a.posObv(c) = P1[3*i + c]; b.posObv(c) = P2[3*i + c]; a.posWorld(c) = b.posWorld(c) = 0.0; }
            for (int c = 0; c < 2; c++) { a.obv2dPred(c) = q1[2*i + c]; b.obv2dPred(c) = q2[2*i + c]; }
            a.obv2d.pt.x = u1[2*i]; a.obv2d.pt.y = u1[2*i + 1]; b.obv2d.pt.x = u2[2*i]; b.obv2d.pt.y = u2[2*i + 1];
            a.FlagTS = b.FlagTS = 0; a.obj = b.obj = 0; a.pt = b.pt = 0; a.KF = b.KF = 0; a.idx2d = b.idx2d = (int)i;
        }
    }
    fclose(f);
    g_lcg = seed;
    tsloop_adapter::PackedSim3Batch P;
    tsloop_adapter::pack_sim3_batch<Traits>(&cur, vKFCands, vvCur, vvCan, K, true, P);
    void *ctx = 0;
    if (tsloop_create(0, &ctx) != TSLOOP_OK) FAIL("tsloop_create");
    tsloop_options o; tsloop_default_options_sim3(&o);
    const int rc = tsloop_sim3_batch(ctx, &P.p, &o);
    if (rc != TSLOOP_OK) { fprintf(stderr, "tsloop_sim3_batch: %d %s\n", rc, tsloop_last_error(ctx)); return 1; }
    FILE *g = fopen(argv[2], "wb"); if (!g) FAIL("cannot open output");
    for (int k = 0; k < nc; k++) {
        const size_t a = (size_t)P.off[(size_t)k], b = (size_t)P.off[(size_t)k + 1], ha = (size_t)P.hyp_off[(size_t)k], hb = (size_t)P.hyp_off[(size_t)k + 1];
        // the reference's loop body from `if(!OK)` on
        std::vector<bool> vbInliers; mock::Sim3_loop gScm; int nInliersOpt = -1;
        const bool OK = tsloop_adapter::scatter_sim3_batch<Traits>(P, (size_t)k, vbInliers, gScm, nInliersOpt);
        if (vbInliers.size() != b - a || OK != (P.ok[(size_t)k] != 0)) FAIL("scatter: sizes");
        int cnt = 0; for (size_t i = 0; i < vbInliers.size(); i++) cnt += vbInliers[i] ? 1 : 0;
        if (OK && (cnt != nInliersOpt || gScm.s != P.sim[8*(size_t)k + 7] || gScm.t(1) != P.sim[8*(size_t)k + 5])) FAIL("scatter: inliers / gScm");
        if (!OK && (cnt != 0 || nInliersOpt != -1)) FAIL("scatter: a discarded candidate");
        const int32_t H = (int32_t)(hb - ha), head[4] = { (int32_t)P.ok[(size_t)k], P.sel[(size_t)k], P.n_inlier_ransac[(size_t)k], (int32_t)nInliersOpt };
        wr(g, &H, 1); wr(g, P.triple.data() + 3*ha, 3*(hb - ha)); wr(g, head, 4);
        wr(g, &P.sim_ransac[8*(size_t)k], 8); wr(g, &P.sim[8*(size_t)k], 8);
        const tsloop_report &r = P.rep[(size_t)k];
        const int32_t ri[4] = { r.iters, r.accepted, r.termination, r.n_inlier }; const double rd2[2] = { r.cost0, r.cost1 };
        wr(g, ri, 4); wr(g, rd2, 2); wr(g, P.inlier.data() + a, b - a); wr(g, P.hyp_count.data() + ha, hb - ha); wr(g, P.hyp_sim.data() + 8*ha, 8*(hb - ha));
    }
    fclose(g);
    tsloop_destroy(ctx);
    printf("sim3 batch from C++: ok\n");
    return 0;
}
