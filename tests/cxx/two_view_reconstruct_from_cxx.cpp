// TEST DRIVER: initializer::ReconstructH / ReconstructF from C++ -- adapter/tsorb_two_view.hpp's reconstruct over mock types of this file.
// Usage: two_view_reconstruct_from_cxx [--host] <in.bin> <out.bin>
//   in : int32 n1, n2, nm, model, min_triangulated; float sigma, min_parallax, M21[9], K[4]; float keys1[n1][2], keys2[n2][2]; int32 matches[nm][2]; uint8 inlier[nm];
//        then for --host the call's outputs to hand on: int32 result[6]; float R21[9], t21[3], p3d[nm][3]; uint8 triangulated[nm]
//   out: int32 n; float xy1[n][2], xy2[n][2]; uint8 inlier[n]; float M21[9], K[4]; int32 ret, hasR, hasT; float R[9], t[3] (zeros where the matrix was left empty);
//        int32 np (= n1 when ret, else 0); float vP3D[np][3]; uint8 vbTriangulated[np];
//        device only: int32 result[6]; float R21[9], t21[3], p3d[n][3]; uint8 triangulated[n] (the call's own outputs)
// --host touches no device: the gather and the filling of the reference's output types from the given outputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "mock_textslam.hpp"
#include "tsorb_two_view.hpp"

struct Mat33f { float m[9]; bool empty; Mat33f() : empty(true) { for (int i = 0; i < 9; i++) m[i] = 0.f; } };          // stands in for cv::Mat (3 x 3, CV_32F)
struct Mat31f { float m[3]; bool empty; Mat31f() : empty(true) { for (int i = 0; i < 3; i++) m[i] = 0.f; } };          // ... (3 x 1, CV_32F)
struct Point3f { float x, y, z; Point3f() : x(0.f), y(0.f), z(0.f) {} };                                               // cv::Point3f
struct Traits { typedef ::Mat33f Mat33f; typedef ::Mat31f Mat31f;
    static void assign33(Mat33f &M, const float m[9]) { for (int i = 0; i < 9; i++) M.m[i] = m[i]; M.empty = false; }
    static void assign31(Mat31f &M, const float m[3]) { for (int i = 0; i < 3; i++) M.m[i] = m[i]; M.empty = false; }
    static float at33(const Mat33f &M, int r, int c) { return M.m[3*r + c]; } };

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "two_view_reconstruct_from_cxx: %s\n", msg); return 1; } while (0)

int main(int argc, char **argv) {
    const bool host = argc > 1 && strcmp(argv[1], "--host") == 0;
    if (argc != (host ? 4 : 3)) FAIL("usage: two_view_reconstruct_from_cxx [--host] in.bin out.bin");
    FILE *f = fopen(argv[host ? 2 : 1], "rb"); if (!f) FAIL("cannot open input");
    int32_t n1 = 0, n2 = 0, nm = 0, model = 0, min_tri = 0; float sigma = 0.f, min_par = 0.f, M[9], Kf[4];
    if (!rd(f, &n1, 1) || !rd(f, &n2, 1) || !rd(f, &nm, 1) || !rd(f, &model, 1) || !rd(f, &min_tri, 1) || !rd(f, &sigma, 1) || !rd(f, &min_par, 1) || !rd(f, M, 9) || !rd(f, Kf, 4) ||
        n1 < 1 || n2 < 1 || nm < 0) FAIL("bad header");
    std::vector<mock::KeyPoint> mvKeys1((size_t)n1), mvKeys2((size_t)n2);
    { std::vector<float> k(2*(size_t)n1); if (!rd(f, k.data(), k.size())) FAIL("short input");
      for (int i = 0; i < n1; i++) { mvKeys1[(size_t)i].pt.x = k[2*(size_t)i]; mvKeys1[(size_t)i].pt.y = k[2*(size_t)i + 1]; } }
    { std::vector<float> k(2*(size_t)n2); if (!rd(f, k.data(), k.size())) FAIL("short input");
      for (int i = 0; i < n2; i++) { mvKeys2[(size_t)i].pt.x = k[2*(size_t)i]; mvKeys2[(size_t)i].pt.y = k[2*(size_t)i + 1]; } }
    std::vector<std::pair<int, int> > mvMatches12((size_t)nm);                                                         // initializer::Match
    { std::vector<int32_t> m(2*(size_t)nm); if (!rd(f, m.data(), m.size())) FAIL("short input");
      for (int i = 0; i < nm; i++) { if (m[2*(size_t)i] < 0 || m[2*(size_t)i] >= n1 || m[2*(size_t)i + 1] < 0 || m[2*(size_t)i + 1] >= n2) FAIL("a match beyond the keypoints");
          mvMatches12[(size_t)i] = std::make_pair((int)m[2*(size_t)i], (int)m[2*(size_t)i + 1]); } }
    std::vector<bool> vbMatchesInliers((size_t)nm);
    { std::vector<uint8_t> b((size_t)nm); if (!rd(f, b.data(), b.size())) FAIL("short input");
      for (int i = 0; i < nm; i++) vbMatchesInliers[(size_t)i] = b[(size_t)i] != 0; }
    Mat33f M21, mK; Traits::assign33(M21, M);
    { const float k[9] = { Kf[0], 0.f, Kf[2], 0.f, Kf[1], Kf[3], 0.f, 0.f, 1.f }; Traits::assign33(mK, k); }
    tsorb_adapter::ReconstructCall c;
    Mat33f R21; Mat31f t21; std::vector<Point3f> vP3D; std::vector<bool> vbTriangulated; bool ret = false;
    void *ctx = 0;
    if (host) {
        c.p3d.resize(3*(size_t)nm); c.triangulated.resize((size_t)nm);
        if (!rd(f, c.result, 6) || !rd(f, c.R21, 9) || !rd(f, c.t21, 3) || !rd(f, c.p3d.data(), c.p3d.size()) || !rd(f, c.triangulated.data(), (size_t)nm)) FAIL("short input");
        fclose(f);
        tsorb_adapter::reconstruct_gather<Traits>(mvKeys1, mvKeys2, mvMatches12, vbMatchesInliers, M21, mK, c);
        ret = tsorb_adapter::reconstruct_fill<Traits>(c, mvMatches12, mvKeys1.size(), R21, t21, vP3D, vbTriangulated);
    } else {
        fclose(f);
        if (tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0) != TSORB_OK) FAIL("tsorb_create");
        ret = tsorb_adapter::reconstruct<Traits>(ctx, mvKeys1, mvKeys2, mvMatches12, vbMatchesInliers, model, M21, mK, sigma, R21, t21, vP3D, vbTriangulated, min_par, min_tri, &c);
        if (!ret && c.result[5] < 0) { fprintf(stderr, "tsorb_match_two_view_reconstruct: %s\n", tsorb_last_error(ctx)); return 1; }
    }
    const int32_t n = c.n(), r = ret ? 1 : 0, hasR = R21.empty ? 0 : 1, hasT = t21.empty ? 0 : 1, np = (int32_t)vP3D.size();
    if (n != nm || (int)c.inlier.size() != n || vbTriangulated.size() != vP3D.size() || (ret && np != n1) || (!ret && np != 0)) FAIL("the gather or the outputs have another length");
    FILE *g = fopen(argv[host ? 3 : 2], "wb"); if (!g) FAIL("cannot open output");
    wr(g, &n, 1); wr(g, c.xy1.data(), c.xy1.size()); wr(g, c.xy2.data(), c.xy2.size()); wr(g, c.inlier.data(), c.inlier.size()); wr(g, c.M21, 9); wr(g, c.K, 4);
    wr(g, &r, 1); wr(g, &hasR, 1); wr(g, &hasT, 1); wr(g, R21.m, 9); wr(g, t21.m, 3); wr(g, &np, 1);
    { std::vector<float> p(3*(size_t)np); std::vector<uint8_t> b((size_t)np);
      for (int i = 0; i < np; i++) { p[3*(size_t)i] = vP3D[(size_t)i].x; p[3*(size_t)i + 1] = vP3D[(size_t)i].y; p[3*(size_t)i + 2] = vP3D[(size_t)i].z; b[(size_t)i] = vbTriangulated[(size_t)i] ? 1 : 0; }
      wr(g, p.data(), p.size()); wr(g, b.data(), b.size()); }
    if (!host) { wr(g, c.result, 6); wr(g, c.R21, 9); wr(g, c.t21, 3); wr(g, c.p3d.data(), 3*(size_t)n); wr(g, c.triangulated.data(), (size_t)n); }
    fclose(g);
    if (ctx) tsorb_destroy(ctx);
    printf(host ? "two view reconstruct from C++ (host): ok\n" : "two view reconstruct from C++: ok\n");
    return 0;
}
