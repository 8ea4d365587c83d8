// TEST INFRASTRUCTURE: frame::FeatExtracText through the adapter (adapter/tsorb_text_extract.hpp) from C++, over mock types.
//
//   text_orb_from_cxx <in.bin> <out.bin>
//     in:  i32 cols, rows, nlevels (of the scene extractor), n_dete; the image (rows x cols u8); n_dete x 4 x 2 f64 corners
//     1. the scene extraction of the frame on one context (ExtractorCore::extract: the upload the text extraction shares);
//     2. the text features of all detections in ONE call, then one detection per call: the two must agree byte for byte;
//     out: per detection i32 count, count x 6 f32 keypoint fields, count x 32 u8 descriptor bytes (of the one call).
//   exit code 0 and "text orb from C++: ok" = all of it.
#include <cstdio>
#include <cstring>
#include <vector>
#include "mock_textslam.hpp"
#include "tsorb_extractor_core.hpp"
#include "tsorb_text_extract.hpp"

struct CvKeyPoint { struct Pt { float x, y; } pt; float size, angle, response; int octave; };       // the fields of cv::KeyPoint the reference reads
struct TextOrbTraits {
    typedef CvKeyPoint KeyPoint;
    typedef mock::Image Mat;                                                                        // cv::Mat CV_8UC1: n rows of 32 bytes
    static KeyPoint keypoint(float x, float y, float size, float angle, float response, int octave) { KeyPoint k; k.pt.x = x; k.pt.y = y; k.size = size; k.angle = angle; k.response = response; k.octave = octave; return k; }
    static Mat descriptors(const uint8_t *rows, int n) { Mat m; m.rows = n; m.cols = n ? 32 : 0; if (n) m.data.assign(rows, rows + 32*(size_t)n); return m; }
};
typedef std::vector<std::vector<mock::Vec2> > Dete;

static bool same(const std::vector<CvKeyPoint> &a, const mock::Image &da, const std::vector<CvKeyPoint> &b, const mock::Image &db) {
    if (a.size() != b.size() || da.rows != db.rows || da.data != db.data) return false;
    for (size_t i = 0; i < a.size(); i++) if (memcmp(&a[i], &b[i], sizeof(CvKeyPoint)) != 0) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int32_t hd[4];
    if (fread(hd, 4, 4, f) != 4 || hd[0] < 1 || hd[1] < 1 || hd[3] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    mock::Image img; img.cols = hd[0]; img.rows = hd[1]; img.data.resize((size_t)hd[0]*hd[1]);
    std::vector<double> q(8*(size_t)hd[3]);
    if (fread(img.data.data(), 1, img.data.size(), f) != img.data.size() || fread(q.data(), 8, q.size(), f) != q.size()) { fprintf(stderr, "input incomplete\n"); return 2; }
    fclose(f);
    Dete TextDete((size_t)hd[3]);
    for (size_t i = 0; i < TextDete.size(); i++) for (int k = 0; k < 4; k++) { mock::Vec2 v; v(0) = q[8*i + 2*k]; v(1) = q[8*i + 2*k + 1]; TextDete[i].push_back(v); }

    tsorb_adapter::ExtractorCore ex(1000, 1.2f, hd[2], 20, 7);                                       // frame::coORBextractor
    if (!ex.ok()) { fprintf(stderr, "tsorb_create: %d\n", ex.create_rc()); return 1; }
    std::vector<float> kps; std::vector<uint8_t> ds;
    const int n_scene = ex.extract(img.data.data(), img.cols, img.rows, img.cols, kps, ds);          // frame::FeatExtraScene: the frame is resident from here on
    if (n_scene < 0) { fprintf(stderr, "extract: %d (%s)\n", n_scene, ex.last_error()); return 1; }

    std::vector<std::vector<CvKeyPoint> > KeysAll; std::vector<mock::Image> DescAll;
    int rc = tsorb_adapter::feat_extrac_text<TextOrbTraits>(ex.tsorb_context(), 0, TextDete, KeysAll, DescAll);
    if (rc != TSORB_OK) { fprintf(stderr, "feat_extrac_text: %d (%s)\n", rc, ex.last_error()); return 1; }
    if (KeysAll.size() != TextDete.size() || DescAll.size() != TextDete.size()) { fprintf(stderr, "wrong number of detections\n"); return 1; }
    size_t total = 0;
    for (size_t i = 0; i < TextDete.size(); i++) {                                                   // the reference's loop: one detection at a time
        Dete one(1, TextDete[i]); std::vector<std::vector<CvKeyPoint> > K1; std::vector<mock::Image> D1;
        rc = tsorb_adapter::feat_extrac_text<TextOrbTraits>(ex.tsorb_context(), 0, one, K1, D1);
        if (rc != TSORB_OK || K1.size() != 1 || D1.size() != 1) { fprintf(stderr, "feat_extrac_text (detection %zu alone): %d\n", i, rc); return 1; }
        if (!same(KeysAll[i], DescAll[i], K1[0], D1[0])) { fprintf(stderr, "detection %zu differs between the one call and its own call\n", i); return 1; }
        if ((int)KeysAll[i].size() != DescAll[i].rows) { fprintf(stderr, "detection %zu: %zu keypoints, %d descriptor rows\n", i, KeysAll[i].size(), DescAll[i].rows); return 1; }
        total += KeysAll[i].size();
    }
    Dete none; std::vector<std::vector<CvKeyPoint> > K0; std::vector<mock::Image> D0;
    if (tsorb_adapter::feat_extrac_text<TextOrbTraits>(ex.tsorb_context(), 0, none, K0, D0) != TSORB_OK || !K0.empty() || !D0.empty()) { fprintf(stderr, "no detection: not empty\n"); return 1; }
    std::vector<float> kps2; std::vector<uint8_t> ds2;                                               // the scene features are still there
    if (ex.extract(img.data.data(), img.cols, img.rows, img.cols, kps2, ds2) != n_scene || kps2 != kps || ds2 != ds) { fprintf(stderr, "scene extraction changed\n"); return 1; }

    FILE *o = fopen(argv[2], "wb"); if (!o) return 2;
    for (size_t i = 0; i < KeysAll.size(); i++) {
        const int32_t n = (int32_t)KeysAll[i].size(); fwrite(&n, 4, 1, o);
        for (int j = 0; j < n; j++) { const CvKeyPoint &k = KeysAll[i][(size_t)j]; const float v[6] = { k.pt.x, k.pt.y, k.size, k.angle, k.response, (float)k.octave }; fwrite(v, 4, 6, o); }
        if (n) fwrite(DescAll[i].data.data(), 1, DescAll[i].data.size(), o);
    }
    fclose(o);
    printf("text orb from C++: ok (%zu detections, %zu text keypoints, %d scene keypoints)\n", TextDete.size(), total, n_scene);
    return 0;
}
