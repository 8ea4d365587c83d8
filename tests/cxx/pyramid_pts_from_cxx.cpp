// TEST INFRASTRUCTURE: frame::TextFeaProc's loop (tsframe_pyramid_pts_batch) driven from C++ through adapter/tsframe_pyramid_pts.hpp over mock
// types with the shape of cv::KeyPoint, Eigen's Vec2 / Mat31 / Mat33 and TextSLAM's TextFeature / SceneFeature.
//
//   pyramid_pts_from_cxx <in.bin> <out.bin>
//     in.bin (tests/test_gpu_pyramid_pts_batch.py): int32 w, h, n_levels, n_dete; double fx, fy, cx, cy; double inv[n_levels]; the image (w x h,
//     8-bit); per detection: int32 m, double PMin.x, PMin.y, PMax.x, PMax.y, m x (float x, y); the scene observations: int32 m, m x (double x, y).
//     1. one context with the pyramid through tsframe_set_image;
//     2. text_fea_proc with the scene set (one call for the frame), then the text-only overload, whose features must be the same;
//     3. writes per detection and level: int32 count, then per feature double u, v, feature(0), feature(1), featureInten, ray(0..2), int32 level,
//        IdxToRaw, uint8 INITIAL, IN; then per level of the scene set: int32 count, per feature double u, v, feature(0), feature(1), int32 level, IdxToRaw.
//   Prints "pyramid pts from C++: ok" and exits 0, 3 without a HIP device, anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tsframe_pyramid_pts.hpp"

namespace mockp {
struct KeyPoint { struct Pt { float x, y; } pt; float size, angle; };
struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat31 { double v[3]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat33 { double m[9]; double operator()(int r, int c) const { return m[3*r + c]; } double &operator()(int r, int c) { return m[3*r + c]; } };
struct TextFeature {                                            // a poisoned constructor: every field the reference sets must be set by the adapter
    double u, v; Vec2 feature; int level, IdxToRaw; bool INITIAL; Mat31 ray; double featureInten, featureNInten; bool IN;
    TextFeature() : u(-1), v(-1), level(-1), IdxToRaw(-1), INITIAL(true), featureInten(-1), featureNInten(-1), IN(true) { feature.v[0] = feature.v[1] = -1; ray.v[0] = ray.v[1] = ray.v[2] = -1; }
};
struct SceneFeature { double u, v; Vec2 feature; int level, IdxToRaw; SceneFeature() : u(-1), v(-1), level(-1), IdxToRaw(-1) { feature.v[0] = feature.v[1] = -1; } };
}  // namespace mockp
using namespace mockp;

template <class T> static bool rd(FILE *f, T *p, size_t k) { return k == 0 || fread(p, sizeof(T), k, f) == k; }
typedef std::vector<std::vector<std::vector<TextFeature *> > > TextPyr;

static bool same(const TextFeature &a, const TextFeature &b) {
    return !memcmp(&a.u, &b.u, 8) && !memcmp(&a.v, &b.v, 8) && !memcmp(a.feature.v, b.feature.v, 16) && a.level == b.level && a.IdxToRaw == b.IdxToRaw &&
           a.INITIAL == b.INITIAL && !memcmp(a.ray.v, b.ray.v, 24) && !memcmp(&a.featureInten, &b.featureInten, 8) && a.IN == b.IN;
}
static void release(TextPyr &p) {
    for (size_t i = 0; i < p.size(); i++) for (size_t l = 0; l < p[i].size(); l++) for (size_t k = 0; k < p[i][l].size(); k++) delete p[i][l][k];
    p.clear();
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    int32_t hd[4]; double kk[4];
    if (!rd(f, hd, 4) || !rd(f, kk, 4)) return 2;
    const int w = hd[0], h = hd[1], nl = hd[2], nd = hd[3];
    if (w < 2 || h < 2 || nl < 1 || nl > TSFRAME_MAX_LEVELS || nd < 0) return 2;
    std::vector<double> inv((size_t)nl);
    std::vector<uint8_t> img((size_t)w*h);
    if (!rd(f, inv.data(), inv.size()) || !rd(f, img.data(), img.size())) return 2;
    std::vector<std::vector<KeyPoint> > vKeysText((size_t)nd);
    std::vector<Vec2> vTextDeteMin((size_t)nd), vTextDeteMax((size_t)nd), SceneObv2d;
    size_t tot = 0;
    for (int i = 0; i < nd; i++) {
        int32_t m; double bx[4];
        if (!rd(f, &m, 1) || m < 0 || !rd(f, bx, 4)) return 2;
        vTextDeteMin[(size_t)i].v[0] = bx[0]; vTextDeteMin[(size_t)i].v[1] = bx[1]; vTextDeteMax[(size_t)i].v[0] = bx[2]; vTextDeteMax[(size_t)i].v[1] = bx[3];
        std::vector<float> xy(2*(size_t)m);
        if (!rd(f, xy.data(), xy.size())) return 2;
        for (int j = 0; j < m; j++) { KeyPoint k; k.pt.x = xy[2*(size_t)j]; k.pt.y = xy[2*(size_t)j + 1]; k.size = 31.f; k.angle = -1.f; vKeysText[(size_t)i].push_back(k); }
        tot += (size_t)m;
    }
    { int32_t m; if (!rd(f, &m, 1) || m < 0) return 2;
      std::vector<double> xy(2*(size_t)m); if (!rd(f, xy.data(), xy.size())) return 2;
      for (int j = 0; j < m; j++) { Vec2 p; p.v[0] = xy[2*(size_t)j]; p.v[1] = xy[2*(size_t)j + 1]; SceneObv2d.push_back(p); } }
    fclose(f);
    Mat33 K0; memset(K0.m, 0, sizeof K0.m); K0(0, 0) = kk[0]; K0(1, 1) = kk[1]; K0(0, 2) = kk[2]; K0(1, 2) = kk[3]; K0(2, 2) = 1.0;

    void *ctx = nullptr;
    if (tsframe_create(0, &ctx) != TSFRAME_OK) { printf("no HIP device\n"); return 3; }
    TextPyr vfeatureText, again, none;
    std::vector<std::vector<SceneFeature *> > vSceneObv2d;
    // a context without an image: an error, and the outputs stay empty
    if (tsframe_adapter::text_fea_proc(ctx, vKeysText, vTextDeteMin, vTextDeteMax, inv, K0, again) == TSFRAME_OK || !again.empty()) { fprintf(stderr, "no error without an image\n"); return 1; }
    if (tsframe_set_image(ctx, img.data(), w, h, nl) != TSFRAME_OK) { fprintf(stderr, "set_image: %s\n", tsframe_last_error(ctx)); return 1; }
    int rc = tsframe_adapter::text_fea_proc(ctx, vKeysText, vTextDeteMin, vTextDeteMax, inv, K0, vfeatureText, SceneObv2d, vSceneObv2d);
    if (rc != TSFRAME_OK) { fprintf(stderr, "tsframe_pyramid_pts_batch (%d): %s\n", rc, tsframe_last_error(ctx)); return 1; }
    rc = tsframe_adapter::text_fea_proc(ctx, vKeysText, vTextDeteMin, vTextDeteMax, inv, K0, again);
    if (rc != TSFRAME_OK) { fprintf(stderr, "text-only overload (%d): %s\n", rc, tsframe_last_error(ctx)); return 1; }
    if (vfeatureText.size() != (size_t)nd || again.size() != (size_t)nd || vSceneObv2d.size() != (size_t)nl) { fprintf(stderr, "outer shape\n"); return 1; }
    for (size_t i = 0; i < vfeatureText.size(); i++) {
        if (vfeatureText[i].size() != (size_t)nl || again[i].size() != (size_t)nl) { fprintf(stderr, "levels of %zu\n", i); return 1; }
        for (size_t l = 0; l < vfeatureText[i].size(); l++) {
            if (vfeatureText[i][l].size() != again[i][l].size()) { fprintf(stderr, "count of %zu level %zu\n", i, l); return 1; }
            for (size_t k = 0; k < vfeatureText[i][l].size(); k++)
                if (!same(*vfeatureText[i][l][k], *again[i][l][k])) { fprintf(stderr, "the text-only overload differs at %zu %zu %zu\n", i, l, k); return 1; }
        }
    }
    // a frame without text detections: no launch, no error
    { std::vector<std::vector<KeyPoint> > k0; std::vector<Vec2> a0, b0;
      if (tsframe_adapter::text_fea_proc(ctx, k0, a0, b0, inv, K0, none) != TSFRAME_OK || !none.empty()) { fprintf(stderr, "empty frame\n"); return 1; } }
    tsframe_destroy(ctx);

    FILE *o = fopen(argv[2], "wb"); if (!o) { perror(argv[2]); return 2; }
    for (size_t i = 0; i < vfeatureText.size(); i++)
        for (size_t l = 0; l < vfeatureText[i].size(); l++) {
            const int32_t m = (int32_t)vfeatureText[i][l].size();
            fwrite(&m, 4, 1, o);
            for (size_t k = 0; k < vfeatureText[i][l].size(); k++) {
                const TextFeature &t = *vfeatureText[i][l][k];
                const double d[8] = { t.u, t.v, t.feature(0), t.feature(1), t.featureInten, t.ray(0), t.ray(1), t.ray(2) };
                const int32_t q[2] = { t.level, t.IdxToRaw }; const uint8_t b[2] = { (uint8_t)t.INITIAL, (uint8_t)t.IN };
                fwrite(d, 8, 8, o); fwrite(q, 4, 2, o); fwrite(b, 1, 2, o);
            }
        }
    for (size_t l = 0; l < vSceneObv2d.size(); l++) {
        const int32_t m = (int32_t)vSceneObv2d[l].size();
        fwrite(&m, 4, 1, o);
        for (size_t k = 0; k < vSceneObv2d[l].size(); k++) {
            const SceneFeature &t = *vSceneObv2d[l][k];
            const double d[4] = { t.u, t.v, t.feature(0), t.feature(1) }; const int32_t q[2] = { t.level, t.IdxToRaw };
            fwrite(d, 8, 4, o); fwrite(q, 4, 2, o);
            delete vSceneObv2d[l][k];
        }
    }
    fclose(o);
    release(vfeatureText); release(again);
    printf("pyramid pts from C++: ok (%d detections, %zu text keypoints, %zu scene observations)\n", nd, tot, SceneObv2d.size());
    return 0;
}
