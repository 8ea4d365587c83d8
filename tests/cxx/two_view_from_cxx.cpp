// TEST DRIVER: initializer::FindHomography + FindFundamental from C++ -- adapter/tsorb_two_view.hpp over mock types of this file.
// Usage: two_view_from_cxx [--host] <in.bin> <out.bin>
//   in : int32 n1, n2, nm, H; float sigma; float keys1[n1][2], keys2[n2][2]; int32 matches[nm][2]; int32 sets[H][8];
//        then for --host the call's outputs to hand on: int32 sel[2]; float score[2], H21[9], F21[9]; uint8 inlier_h[nm], inlier_f[nm]
//   out: float norm1[4], norm2[4]; int32 n; float xy1[n][2], xy2[n][2]; int32 H; int32 subset[H][8];
//        int32 ret; float SH, SF; int32 hasH, hasF; float Hm[9], Fm[9] (zeros where the matrix was left empty); uint8 inlH[n], inlF[n] (the vector<bool>s);
//        device only: int32 sel[2]
// --host touches no device: Normalize's statistics, the gather and the filling of the reference's output types from the given outputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "mock_textslam.hpp"
#include "tsorb_two_view.hpp"

struct Mat33f { float m[9]; bool empty; Mat33f() : empty(true) { for (int i = 0; i < 9; i++) m[i] = 0.f; } };          // stands in for cv::Mat (3 x 3, CV_32F)
struct Traits { typedef ::Mat33f Mat33f; static void assign33(Mat33f &M, const float m[9]) { for (int i = 0; i < 9; i++) M.m[i] = m[i]; M.empty = false; } };

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "two_view_from_cxx: %s\n", msg); return 1; } while (0)

int main(int argc, char **argv) {
    const bool host = argc > 1 && strcmp(argv[1], "--host") == 0;
    if (argc != (host ? 4 : 3)) FAIL("usage: two_view_from_cxx [--host] in.bin out.bin");
    FILE *f = fopen(argv[host ? 2 : 1], "rb"); if (!f) FAIL("cannot open input");
    int32_t n1 = 0, n2 = 0, nm = 0, H = 0; float sigma = 0.f;
    if (!rd(f, &n1, 1) || !rd(f, &n2, 1) || !rd(f, &nm, 1) || !rd(f, &H, 1) || !rd(f, &sigma, 1) || n1 < 1 || n2 < 1 || nm < 0 || H < 0) FAIL("bad header");
    std::vector<mock::KeyPoint> mvKeys1((size_t)n1), mvKeys2((size_t)n2);
    { std::vector<float> k(2*(size_t)n1); if (!rd(f, k.data(), k.size())) FAIL("short input");
      for (int i = 0; i < n1; i++) { mvKeys1[(size_t)i].pt.x = k[2*(size_t)i]; mvKeys1[(size_t)i].pt.y = k[2*(size_t)i + 1]; } }
    { std::vector<float> k(2*(size_t)n2); if (!rd(f, k.data(), k.size())) FAIL("short input");
      for (int i = 0; i < n2; i++) { mvKeys2[(size_t)i].pt.x = k[2*(size_t)i]; mvKeys2[(size_t)i].pt.y = k[2*(size_t)i + 1]; } }
    std::vector<std::pair<int, int> > mvMatches12((size_t)nm);                                                         // initializer::Match
    { std::vector<int32_t> m(2*(size_t)nm); if (!rd(f, m.data(), m.size())) FAIL("short input");
      for (int i = 0; i < nm; i++) { if (m[2*(size_t)i] < 0 || m[2*(size_t)i] >= n1 || m[2*(size_t)i + 1] < 0 || m[2*(size_t)i + 1] >= n2) FAIL("a match beyond the keypoints");
          mvMatches12[(size_t)i] = std::make_pair((int)m[2*(size_t)i], (int)m[2*(size_t)i + 1]); } }
    std::vector<std::vector<size_t> > mvSets((size_t)H, std::vector<size_t>(8, 0));
    { std::vector<int32_t> s(8*(size_t)H); if (!rd(f, s.data(), s.size())) FAIL("short input");
      for (int h = 0; h < H; h++) for (int j = 0; j < 8; j++) mvSets[(size_t)h][(size_t)j] = (size_t)s[8*(size_t)h + j]; }
    tsorb_adapter::TwoViewCall c;
    std::vector<bool> inlH, inlF; float SH = -1.f, SF = -1.f; Mat33f Hm, Fm; bool ret = false;
    void *ctx = 0;
    if (host) {
        c.inlier_h.resize((size_t)nm); c.inlier_f.resize((size_t)nm);
        if (!rd(f, c.sel, 2) || !rd(f, c.score, 2) || !rd(f, c.H21, 9) || !rd(f, c.F21, 9) || !rd(f, c.inlier_h.data(), (size_t)nm) || !rd(f, c.inlier_f.data(), (size_t)nm)) FAIL("short input");
        fclose(f);
        tsorb_adapter::two_view_gather(mvKeys1, mvKeys2, mvMatches12, mvSets, c);
        tsorb_adapter::two_view_normalize(mvKeys1, c.norm1); tsorb_adapter::two_view_normalize(mvKeys2, c.norm2);
        ret = tsorb_adapter::two_view_fill<Traits>(c, inlH, SH, Hm, inlF, SF, Fm);
    } else {
        fclose(f);
        if (tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0) != TSORB_OK) FAIL("tsorb_create");
        ret = tsorb_adapter::find_h_and_f<Traits>(ctx, mvKeys1, mvKeys2, mvMatches12, mvSets, sigma, inlH, SH, Hm, inlF, SF, Fm, 0, &c);
        if (!ret && inlH.empty()) { fprintf(stderr, "tsorb_match_two_view_ransac: %s\n", tsorb_last_error(ctx)); return 1; }
    }
    const int32_t n = c.n(), Hs = c.n_hyp(), r = ret ? 1 : 0, hasH = Hm.empty ? 0 : 1, hasF = Fm.empty ? 0 : 1;
    if (n != nm || (int)inlH.size() != n || (int)inlF.size() != n) FAIL("the gather or the masks have another length");
    for (int i = 0; i < n; i++) {                                                                                      // the gather against a plain transcription
        if (c.xy1[2*(size_t)i] != mvKeys1[(size_t)mvMatches12[(size_t)i].first].pt.x || c.xy1[2*(size_t)i + 1] != mvKeys1[(size_t)mvMatches12[(size_t)i].first].pt.y ||
            c.xy2[2*(size_t)i] != mvKeys2[(size_t)mvMatches12[(size_t)i].second].pt.x || c.xy2[2*(size_t)i + 1] != mvKeys2[(size_t)mvMatches12[(size_t)i].second].pt.y)
            FAIL("the gather is not the transcription's"); }
    FILE *g = fopen(argv[host ? 3 : 2], "wb"); if (!g) FAIL("cannot open output");
    wr(g, c.norm1, 4); wr(g, c.norm2, 4); wr(g, &n, 1); wr(g, c.xy1.data(), c.xy1.size()); wr(g, c.xy2.data(), c.xy2.size()); wr(g, &Hs, 1); wr(g, c.subset.data(), c.subset.size());
    wr(g, &r, 1); wr(g, &SH, 1); wr(g, &SF, 1); wr(g, &hasH, 1); wr(g, &hasF, 1); wr(g, Hm.m, 9); wr(g, Fm.m, 9);
    { std::vector<uint8_t> a((size_t)n), b((size_t)n); for (int i = 0; i < n; i++) { a[(size_t)i] = inlH[(size_t)i] ? 1 : 0; b[(size_t)i] = inlF[(size_t)i] ? 1 : 0; }
      wr(g, a.data(), a.size()); wr(g, b.data(), b.size()); }
    if (!host) wr(g, c.sel, 2);
    fclose(g);
    if (ctx) tsorb_destroy(ctx);
    printf(host ? "two view from C++ (host): ok\n" : "two view from C++: ok\n");
    return 0;
}
