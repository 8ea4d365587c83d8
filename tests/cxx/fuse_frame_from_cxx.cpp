// TEST INFRASTRUCTURE: frame::FeatExtract's steps 3 - 4 + frame::FeatFusion through the adapter (adapter/tsorb_fuse_frame.hpp) from C++, over mock types, and a plain
// host transcription of tool::BoundFeatDele_T + frame::FeatFusion through the same polygon test (textslam_amd/csrc/tsfuse.h).
//
//   fuse_frame_from_cxx <in.bin> <out.bin>                    (needs a device; not compiled with -DFUSE_HOST_ONLY)
//     in:  i32 cols, rows, nlevels (of the scene extractor), n_dete; the image (rows x cols u8); n_dete x 4 x 2 f64 corners; n_dete x 4 f64 vTextDeteMin x, y,
//          vTextDeteMax x, y; 4 f64 mnMinX, mnMaxX, mnMinY, mnMaxY
//     1. the scene extraction of the frame on one context (ExtractorCore::extract);
//     2. feat_extract_fuse, then once more with room for one scene row only (the retry with the reported counts): the two must agree;
//     3. the scene extraction once more: unchanged.
//   fuse_frame_from_cxx --host <in.bin> <out.bin>             (no device)
//     in:  i32 n_scene, n_dete; n_scene x 6 f32, n_scene x 32 u8; n_dete x 4 x 2 f64; n_dete x 4 f64; f64 win; per detection i32 k, k x 6 f32, k x 32 u8 (the raw text features)
//   out (both): i32 iNScene, iNTextObj, iNTextFea, iN; vKeysScene (iNScene x 6 f32), mDescrScene (iNScene x 32 u8); per detection i32 k, vKeysText (k x 6 f32),
//     mDescrText (k x 32 u8), vKeysTextIdx (k i32), IdxNewText (k i32); vKeys (iN x 6 f32), mDescr (iN x 32 u8), vTextObjInfo (iN i32), vKeysSceneIdx (iNScene i32)
//   exit code 0 and "fuse frame from C++: ok" = all of it.
#include <cstdio>
#include <cstring>
#include <vector>
#include "mock_textslam.hpp"
#include "tsfuse.h"
#ifndef FUSE_HOST_ONLY
#include "tsorb_extractor_core.hpp"
#endif
#include "tsorb_fuse_frame.hpp"

struct CvKeyPoint { struct Pt { float x, y; } pt; float size, angle, response; int octave; };       // the fields of cv::KeyPoint the reference reads
struct TextOrbTraits {
    typedef CvKeyPoint KeyPoint;
    typedef mock::Image Mat;                                                                        // cv::Mat CV_8UC1: n rows of 32 bytes
    static KeyPoint keypoint(float x, float y, float size, float angle, float response, int octave) { KeyPoint k; k.pt.x = x; k.pt.y = y; k.size = size; k.angle = angle; k.response = response; k.octave = octave; return k; }
    static Mat descriptors(const uint8_t *rows, int n) { Mat m; m.rows = n; m.cols = n ? 32 : 0; if (n) m.data.assign(rows, rows + 32*(size_t)n); return m; }
};
typedef tsorb_adapter::FusedFrame<TextOrbTraits> Fused;
typedef std::vector<std::vector<mock::Vec2> > Dete;

static bool read_n(FILE *f, void *p, size_t size, size_t n) { return n == 0 || fread(p, size, n, f) == n; }
static void put_keys(FILE *o, const std::vector<CvKeyPoint> &K) {
    for (size_t j = 0; j < K.size(); j++) { const CvKeyPoint &k = K[j]; const float v[6] = { k.pt.x, k.pt.y, k.size, k.angle, k.response, (float)k.octave }; fwrite(v, 4, 6, o); } }
static void put_mat(FILE *o, const mock::Image &m) { if (!m.data.empty()) fwrite(m.data.data(), 1, m.data.size(), o); }
static bool dump(const char *path, const Fused &F) {
    FILE *o = fopen(path, "wb"); if (!o) return false;
    const int32_t hd[4] = { F.iNScene, F.iNTextObj, F.iNTextFea, F.iN }; fwrite(hd, 4, 4, o);
    put_keys(o, F.vKeysScene); put_mat(o, F.mDescrScene);
    for (size_t i = 0; i < F.vKeysText.size(); i++) {
        const int32_t k = (int32_t)F.vKeysText[i].size(); fwrite(&k, 4, 1, o);
        put_keys(o, F.vKeysText[i]); put_mat(o, F.mDescrText[i]);
        for (size_t j = 0; j < F.vKeysTextIdx[i].size(); j++) { const int32_t v = (int32_t)F.vKeysTextIdx[i][j]; fwrite(&v, 4, 1, o); }
        for (size_t j = 0; j < F.IdxNewText[i].size(); j++) { const int32_t v = F.IdxNewText[i][j]; fwrite(&v, 4, 1, o); }
    }
    put_keys(o, F.vKeys); put_mat(o, F.mDescr);
    for (size_t j = 0; j < F.vTextObjInfo.size(); j++) { const int32_t v = F.vTextObjInfo[j]; fwrite(&v, 4, 1, o); }
    for (size_t j = 0; j < F.vKeysSceneIdx.size(); j++) { const int32_t v = (int32_t)F.vKeysSceneIdx[j]; fwrite(&v, 4, 1, o); }
    return fclose(o) == 0;
}
static bool consistent(const Fused &F) {                                                             // the reference's own check (frame.cc:320) and the sizes
    size_t text = 0; for (size_t i = 0; i < F.vKeysText.size(); i++) { text += F.vKeysText[i].size();
        if ((int)F.vKeysText[i].size() != F.mDescrText[i].rows || F.vKeysTextIdx[i].size() != F.vKeysText[i].size() || F.IdxNewText[i].size() != F.vKeysText[i].size()) return false; }
    return F.iN == F.iNScene + F.iNTextFea && (size_t)F.iNTextFea == text && F.iN == F.mDescr.rows && F.iNScene == F.mDescrScene.rows && (size_t)F.iNTextObj == F.mDescrText.size() &&
           (size_t)F.iN == F.vKeys.size() && (size_t)F.iN == F.vTextObjInfo.size() && (size_t)F.iNScene == F.vKeysSceneIdx.size() && (size_t)F.iNScene == F.vKeysScene.size();
}
static std::vector<CvKeyPoint> keys_of(const std::vector<float> &kp) {
    std::vector<CvKeyPoint> K; for (size_t j = 0; j + 5 < kp.size(); j += 6) K.push_back(TextOrbTraits::keypoint(kp[j], kp[j + 1], kp[j + 2], kp[j + 3], kp[j + 4], (int)kp[j + 5])); return K; }

// tool::BoundFeatDele_T (src/tool.cc:456-508) + frame::FeatFusion (src/frame.cc:257-325), as written there, over the raw features
static void host_fuse(const std::vector<CvKeyPoint> &KeysSceneRaw, const mock::Image &DescripSceneRaw, const std::vector<std::vector<CvKeyPoint> > &KeysTextRaw,
                      const std::vector<mock::Image> &DescripTextRaw, const std::vector<double> &quad, const std::vector<double> &bbox, double win, Fused &F) {
    F = Fused();
    for (size_t i0 = 0; i0 < KeysTextRaw.size(); i0++) {
        int polys[16]; fuse_shrunk_quad(&quad[8*i0], win, polys); fuse_bbox_quad(&bbox[4*i0], polys + 8);          // GetNewDeteBox, GetbbDeteBox, vV2vP
        std::vector<CvKeyPoint> cell; std::vector<uint8_t> rows; std::vector<int> idx;
        for (size_t r = 0; r < KeysTextRaw[i0].size(); r++) { const CvKeyPoint &fea = KeysTextRaw[i0][r];
            if (!fuse_point_in_polygon(polys, 4, fea.pt.x, fea.pt.y) || !fuse_point_in_polygon(polys + 8, 4, fea.pt.x, fea.pt.y)) continue;
            cell.push_back(fea); rows.insert(rows.end(), DescripTextRaw[i0].data.begin() + 32*r, DescripTextRaw[i0].data.begin() + 32*(r + 1)); idx.push_back((int)r); }
        F.vKeysText.push_back(cell); F.mDescrText.push_back(TextOrbTraits::descriptors(rows.data(), (int)cell.size())); F.IdxNewText.push_back(idx);
    }
    F.vKeysScene = KeysSceneRaw; F.mDescrScene = DescripSceneRaw;
    F.iNScene = (int)F.vKeysScene.size(); F.iNTextObj = (int)F.vKeysText.size(); F.iNTextFea = 0;
    std::vector<uint8_t> all(F.mDescrScene.data);
    for (int i0 = 0; i0 < F.iNTextObj; i0++) { F.iNTextFea += (int)F.vKeysText[(size_t)i0].size(); all.insert(all.end(), F.mDescrText[(size_t)i0].data.begin(), F.mDescrText[(size_t)i0].data.end()); }
    F.iN = F.iNScene + F.iNTextFea;
    F.mDescr = TextOrbTraits::descriptors(all.data(), F.iN);
    F.vKeys.resize((size_t)F.iN); F.vKeysSceneIdx.resize((size_t)F.iNScene); F.vKeysTextIdx.resize((size_t)F.iNTextObj); F.vTextObjInfo = std::vector<int>((size_t)F.iN, -1);
    for (int i1 = 0; i1 < F.iNScene; i1++) { F.vKeys[(size_t)i1] = F.vKeysScene[(size_t)i1]; F.vKeysSceneIdx[(size_t)i1] = (size_t)i1; }
    int IdxBeginText = F.iNScene, IdxText = 0;
    for (int i2 = 0; i2 < F.iNTextObj; i2++) { const std::vector<CvKeyPoint> &cell = F.vKeysText[(size_t)i2];
        F.vKeysTextIdx[(size_t)i2].resize(cell.size());
        for (size_t i3 = 0; i3 < cell.size(); i3++) { const int IdxFea = IdxText + IdxBeginText; F.vKeys[(size_t)IdxFea] = cell[i3]; F.vTextObjInfo[(size_t)IdxFea] = i2; F.vKeysTextIdx[(size_t)i2][i3] = (size_t)IdxFea; IdxText++; } }
}

static int host_mode(const char *in, const char *out) {
    FILE *f = fopen(in, "rb"); if (!f) { fprintf(stderr, "cannot read %s\n", in); return 2; }
    int32_t hd[2];
    if (fread(hd, 4, 2, f) != 2 || hd[0] < 0 || hd[1] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t ns = (size_t)hd[0], nd = (size_t)hd[1];
    std::vector<float> skp(6*ns); std::vector<uint8_t> sde(32*ns); std::vector<double> quad(8*nd), bbox(4*nd); double win = 0;
    if (!read_n(f, skp.data(), 4, skp.size()) || !read_n(f, sde.data(), 1, sde.size()) || !read_n(f, quad.data(), 8, quad.size()) || !read_n(f, bbox.data(), 8, bbox.size()) || fread(&win, 8, 1, f) != 1) { fprintf(stderr, "input incomplete\n"); return 2; }
    std::vector<std::vector<CvKeyPoint> > KeysTextRaw(nd); std::vector<mock::Image> DescripTextRaw(nd);
    for (size_t i = 0; i < nd; i++) { int32_t k = 0; if (fread(&k, 4, 1, f) != 1 || k < 0) { fprintf(stderr, "input incomplete\n"); return 2; }
        std::vector<float> kp(6*(size_t)k); std::vector<uint8_t> de(32*(size_t)k);
        if (!read_n(f, kp.data(), 4, kp.size()) || !read_n(f, de.data(), 1, de.size())) { fprintf(stderr, "input incomplete\n"); return 2; }
        KeysTextRaw[i] = keys_of(kp); DescripTextRaw[i] = TextOrbTraits::descriptors(de.data(), k); }
    fclose(f);
    Fused F;
    host_fuse(keys_of(skp), TextOrbTraits::descriptors(sde.data(), (int)ns), KeysTextRaw, DescripTextRaw, quad, bbox, win, F);
    if (!consistent(F)) { fprintf(stderr, "error: Keys number is not same.\n"); return 1; }
    if (!dump(out, F)) return 2;
    printf("fuse frame from C++: ok (host; %d scene + %d text features of %d detections)\n", F.iNScene, F.iNTextFea, F.iNTextObj);
    return 0;
}

#ifndef FUSE_HOST_ONLY
static bool same_keys(const std::vector<CvKeyPoint> &a, const std::vector<CvKeyPoint> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (memcmp(&a[i], &b[i], sizeof(CvKeyPoint)) != 0) return false;
    return true; }
static bool same(const Fused &A, const Fused &B) {
    if (A.iNScene != B.iNScene || A.iNTextObj != B.iNTextObj || A.iNTextFea != B.iNTextFea || A.iN != B.iN || !same_keys(A.vKeys, B.vKeys) || A.mDescr.data != B.mDescr.data ||
        !same_keys(A.vKeysScene, B.vKeysScene) || A.mDescrScene.data != B.mDescrScene.data || A.vTextObjInfo != B.vTextObjInfo || A.vKeysSceneIdx != B.vKeysSceneIdx ||
        A.vKeysTextIdx != B.vKeysTextIdx || A.IdxNewText != B.IdxNewText) return false;
    for (size_t i = 0; i < A.vKeysText.size(); i++) if (!same_keys(A.vKeysText[i], B.vKeysText[i]) || A.mDescrText[i].data != B.mDescrText[i].data) return false;
    return true; }

static int device_mode(const char *in, const char *out) {
    FILE *f = fopen(in, "rb"); if (!f) { fprintf(stderr, "cannot read %s\n", in); return 2; }
    int32_t hd[4];
    if (fread(hd, 4, 4, f) != 4 || hd[0] < 1 || hd[1] < 1 || hd[3] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    mock::Image img; img.cols = hd[0]; img.rows = hd[1]; img.data.resize((size_t)hd[0]*hd[1]);
    const size_t nd = (size_t)hd[3];
    std::vector<double> q(8*nd), bb(4*nd); double bounds[4];
    if (fread(img.data.data(), 1, img.data.size(), f) != img.data.size() || !read_n(f, q.data(), 8, q.size()) || !read_n(f, bb.data(), 8, bb.size()) || fread(bounds, 8, 4, f) != 4) { fprintf(stderr, "input incomplete\n"); return 2; }
    fclose(f);
    Dete TextDete(nd); std::vector<mock::Vec2> vTextDeteMin(nd), vTextDeteMax(nd);
    for (size_t i = 0; i < nd; i++) { for (int k = 0; k < 4; k++) { mock::Vec2 v; v(0) = q[8*i + 2*k]; v(1) = q[8*i + 2*k + 1]; TextDete[i].push_back(v); }
        vTextDeteMin[i](0) = bb[4*i]; vTextDeteMin[i](1) = bb[4*i + 1]; vTextDeteMax[i](0) = bb[4*i + 2]; vTextDeteMax[i](1) = bb[4*i + 3]; }

    tsorb_adapter::ExtractorCore ex(1000, 1.2f, hd[2], 20, 7);                                       // frame::coORBextractor
    if (!ex.ok()) { fprintf(stderr, "tsorb_create: %d\n", ex.create_rc()); return 1; }
    std::vector<float> kps; std::vector<uint8_t> ds;
    const int n_scene = ex.extract(img.data.data(), img.cols, img.rows, img.cols, kps, ds);          // frame::FeatExtraScene: the frame is resident from here on
    if (n_scene < 0) { fprintf(stderr, "extract: %d (%s)\n", n_scene, ex.last_error()); return 1; }

    Fused F, G;
    int rc = tsorb_adapter::feat_extract_fuse<TextOrbTraits>(ex.tsorb_context(), 0, TextDete, vTextDeteMin, vTextDeteMax, bounds, F);
    if (rc != TSORB_OK) { fprintf(stderr, "feat_extract_fuse: %d (%s)\n", rc, ex.last_error()); return 1; }
    if (!consistent(F) || F.iNScene != n_scene || (size_t)F.iNTextObj != nd) { fprintf(stderr, "error: Keys number is not same.\n"); return 1; }
    if (!same_keys(F.vKeysScene, keys_of(kps)) || F.mDescrScene.data != ds) { fprintf(stderr, "the scene rows are not the scene extraction's\n"); return 1; }
    rc = tsorb_adapter::feat_extract_fuse<TextOrbTraits>(ex.tsorb_context(), 0, TextDete, vTextDeteMin, vTextDeteMax, bounds, G, 500, -3.0, 1);      // room for one scene row: the retry
    if (rc != TSORB_OK) { fprintf(stderr, "feat_extract_fuse (retry): %d (%s)\n", rc, ex.last_error()); return 1; }
    if (!same(F, G)) { fprintf(stderr, "the retry with the reported counts differs\n"); return 1; }
    std::vector<float> kps2; std::vector<uint8_t> ds2;                                               // the scene features are still there
    if (ex.extract(img.data.data(), img.cols, img.rows, img.cols, kps2, ds2) != n_scene || kps2 != kps || ds2 != ds) { fprintf(stderr, "scene extraction changed\n"); return 1; }
    if (!dump(out, F)) return 2;
    printf("fuse frame from C++: ok (%d scene + %d text features of %d detections)\n", F.iNScene, F.iNTextFea, F.iNTextObj);
    return 0;
}
#endif

int main(int argc, char **argv) {
    if (argc == 4 && strcmp(argv[1], "--host") == 0) return host_mode(argv[2], argv[3]);
#ifndef FUSE_HOST_ONLY
    if (argc == 3) return device_mode(argv[1], argv[2]);
#endif
    fprintf(stderr, "usage: %s [--host] in.bin out.bin\n", argv[0]); return 2;
}
