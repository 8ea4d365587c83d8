// TEST DRIVER: tracking::CheckMatch from C++ -- adapter/tsorb_pnp_check.hpp over mock types of this file (the math structs are mock_textslam.hpp's).
// Usage: pnp_check_from_cxx [--host] <in.bin> <out.bin>
//   in : int32 n_kf, n_pts, n_keys; double mK[9]; float ReproError; double Twc[n_kf][16]; per point: int32 kf, double ray[3], double rho; int32 vMatch3D2D[n_pts];
//        float keys[n_keys][2]; then for --host: int32 ok, int32 n_mask, uint8 mask[n_mask]
//   out: int32 n; float Pw[n][3], uv[n][2]; double K[4]; int32 H, subset[H][5]; then
//        device: int32 called, ret; int32 result[4]; double pose[12]; int32 hyp_count[H]; uint8 inlier[n]; int32 vMatch3D2D[n_pts]
//        --host: int32 ret; int32 vMatch3D2D[n_pts]          (the given mask applied; nothing touches a device)
// Both modes hold the gather and the application of the mask equal to a plain transcription of CheckMatch's own loops (:1503-1529, :1561-1576) before they write.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mock_textslam.hpp"
#include "tsorb_pnp_check.hpp"

struct KeyFrame { mock::Mat44 Twc; mock::Mat44 GetTwc() const { return Twc; } };
struct MapPt { KeyFrame *RefKF; mock::Mat31 ray; double rho; mock::Mat31 GetRaydir() const { return ray; } double GetInverD() const { return rho; } };
struct Frame { std::vector<mock::KeyPoint> vKeys; mock::Mat33 mK; };

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "pnp_check_from_cxx: %s\n", msg); return 1; } while (0)

// CheckMatch's first loop, transcribed: vP3d (as the floats solvePnPRansac works on) and vP2d
static void plain_gather(const std::vector<MapPt *> &Pts3d, const Frame &F, const std::vector<int> &vMatch3D2D, std::vector<float> &vP3d, std::vector<float> &vP2d) {
    for (size_t imatch = 0; imatch < vMatch3D2D.size(); imatch++) {
        if (vMatch3D2D[imatch] < 0)
            continue;
        int idx1 = (int)imatch;
        int idx2 = vMatch3D2D[imatch];
        MapPt *pt = Pts3d[(size_t)idx1];
        mock::Mat44 Twr = pt->RefKF->GetTwc();
        mock::Mat31 ray = pt->GetRaydir();
        double rho = pt->GetInverD();
        double pw[3];
        for (int r = 0; r < 3; r++) pw[r] = (Twr(r, 0)*ray(0) + Twr(r, 1)*ray(1) + Twr(r, 2)*ray(2))/rho + Twr(r, 3);
        vP3d.push_back((float)pw[0]); vP3d.push_back((float)pw[1]); vP3d.push_back((float)pw[2]);
        vP2d.push_back((float)F.vKeys[(size_t)idx2].pt.x); vP2d.push_back((float)F.vKeys[(size_t)idx2].pt.y);
    }
}
// CheckMatch's last loop, transcribed, from the inlier index list solvePnPRansac returns (empty when it fails)
static int plain_update(const std::vector<int> &inliers, std::vector<int> &vMatch3D2D, size_t n) {
    std::vector<bool> PnPres(n, false);
    for (size_t i = 0; i < inliers.size(); i++) PnPres[(size_t)inliers[i]] = true;
    int numMatch = (int)n, idx = -1;
    for (size_t iupdate = 0; iupdate < vMatch3D2D.size(); iupdate++) {
        if (vMatch3D2D[iupdate] < 0)
            continue;
        idx++;
        if (PnPres[(size_t)idx])
            continue;
        vMatch3D2D[iupdate] = -1;
        numMatch--;
    }
    return numMatch;
}

int main(int argc, char **argv) {
    const bool host = argc > 1 && strcmp(argv[1], "--host") == 0;
    if (argc != (host ? 4 : 3)) FAIL("usage: pnp_check_from_cxx [--host] in.bin out.bin");
    FILE *f = fopen(argv[host ? 2 : 1], "rb"); if (!f) FAIL("cannot open input");
    int32_t n_kf = 0, n_pts = 0, n_keys = 0; Frame F; float ReproError = 0.f;
    if (!rd(f, &n_kf, 1) || !rd(f, &n_pts, 1) || !rd(f, &n_keys, 1) || !rd(f, F.mK.m, 9) || !rd(f, &ReproError, 1) || n_kf < 1 || n_pts < 0 || n_keys < 0) FAIL("bad header");
    std::vector<KeyFrame> kfs((size_t)n_kf); std::vector<MapPt> pts((size_t)n_pts); std::vector<MapPt *> Pts3d; std::vector<int> vMatch3D2D((size_t)n_pts);
    for (int k = 0; k < n_kf; k++) if (!rd(f, kfs[(size_t)k].Twc.m, 16)) FAIL("short input");
    for (int i = 0; i < n_pts; i++) { int32_t kf = 0;
        if (!rd(f, &kf, 1) || !rd(f, pts[(size_t)i].ray.v, 3) || !rd(f, &pts[(size_t)i].rho, 1) || kf < 0 || kf >= n_kf) FAIL("short input");
        pts[(size_t)i].RefKF = &kfs[(size_t)kf]; Pts3d.push_back(&pts[(size_t)i]); }
    { std::vector<int32_t> m((size_t)n_pts); if (!rd(f, m.data(), m.size())) FAIL("short input");
      for (int i = 0; i < n_pts; i++) { if (m[(size_t)i] >= n_keys) FAIL("a match beyond the keypoints"); vMatch3D2D[(size_t)i] = m[(size_t)i]; } }
    { std::vector<float> k(2*(size_t)n_keys); if (!rd(f, k.data(), k.size())) FAIL("short input");
      F.vKeys.resize((size_t)n_keys); for (int i = 0; i < n_keys; i++) { F.vKeys[(size_t)i].pt.x = k[2*(size_t)i]; F.vKeys[(size_t)i].pt.y = k[2*(size_t)i + 1]; } }
    int32_t given_ok = 0, n_mask = 0; std::vector<uint8_t> given;
    if (host) { if (!rd(f, &given_ok, 1) || !rd(f, &n_mask, 1) || n_mask < 0) FAIL("short input"); given.resize((size_t)n_mask); if (!rd(f, given.data(), given.size())) FAIL("short input"); }
    fclose(f);

    std::vector<float> vP3d, vP2d; plain_gather(Pts3d, F, vMatch3D2D, vP3d, vP2d);
    const std::vector<int> before = vMatch3D2D; std::vector<int> plain = vMatch3D2D;
    tsorb_adapter::PnpCheckCall c;
    FILE *g = fopen(argv[host ? 3 : 2], "wb"); if (!g) FAIL("cannot open output");
    if (host) {
        tsorb_adapter::pnp_gather(Pts3d, F, vMatch3D2D, c);
        const int32_t n = c.n();
        if (c.Pw != vP3d || c.uv != vP2d) FAIL("the gather is not the transcription's");
        if (n_mask != n) FAIL("the given mask has another length");
        tsorb_adapter::PnpTraits::pnp_subsets(n, 100, c.subset);
        const int32_t H = (int32_t)(c.subset.size()/5);
        const int32_t ret = tsorb_adapter::pnp_apply_mask(given.data(), given_ok != 0, vMatch3D2D);
        std::vector<int> inliers; if (given_ok) for (int i = 0; i < n; i++) if (given[(size_t)i]) inliers.push_back(i);
        if (plain_update(inliers, plain, (size_t)n) != ret || plain != vMatch3D2D) FAIL("the mask's application is not the transcription's");
        wr(g, &n, 1); wr(g, c.Pw.data(), c.Pw.size()); wr(g, c.uv.data(), c.uv.size()); wr(g, c.K, 4); wr(g, &H, 1); wr(g, c.subset.data(), c.subset.size());
        wr(g, &ret, 1); { std::vector<int32_t> m(vMatch3D2D.begin(), vMatch3D2D.end()); wr(g, m.data(), m.size()); }
        fclose(g);
        printf("pnp check from C++ (host): ok\n");
        return 0;
    }
    void *ctx = 0;
    if (tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0) != TSORB_OK) FAIL("tsorb_create");
    bool called = false;
    const int32_t ret = tsorb_adapter::check_match<tsorb_adapter::PnpTraits>(ctx, Pts3d, F, vMatch3D2D, ReproError, called, &c);
    const int32_t n = c.n(), H = (int32_t)(c.subset.size()/5), was_called = called ? 1 : 0;
    if (c.Pw != vP3d || c.uv != vP2d) FAIL("the gather is not the transcription's");
    if (!called) { if (vMatch3D2D != before || ret != -1) FAIL("a call that was not made changed the matches"); }
    else {
        if (ret < 0) { fprintf(stderr, "tsorb_match_pnp_ransac: %s\n", tsorb_last_error(ctx)); return 1; }
        std::vector<int> inliers; if (c.result[0]) for (int i = 0; i < n; i++) if (c.inlier[(size_t)i]) inliers.push_back(i);
        if (plain_update(inliers, plain, (size_t)n) != ret || plain != vMatch3D2D) FAIL("the mask's application is not the transcription's");
        if (c.result[0] && ret != c.result[1]) FAIL("numMatch is not the inlier count");
    }
    wr(g, &n, 1); wr(g, c.Pw.data(), c.Pw.size()); wr(g, c.uv.data(), c.uv.size()); wr(g, c.K, 4); wr(g, &H, 1); wr(g, c.subset.data(), c.subset.size());
    wr(g, &was_called, 1); wr(g, &ret, 1);
    if (called) { wr(g, c.result, 4); wr(g, c.pose, 12); wr(g, c.hyp_count.data(), c.hyp_count.size()); wr(g, c.inlier.data(), c.inlier.size()); }
    { std::vector<int32_t> m(vMatch3D2D.begin(), vMatch3D2D.end()); wr(g, m.data(), m.size()); }
    fclose(g);
    tsorb_destroy(ctx);
    printf("pnp check from C++: ok\n");
    return 0;
}
