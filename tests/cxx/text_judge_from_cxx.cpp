// TEST INFRASTRUCTURE: tracking::TextJudgeSingle for a frame's planes (tsframe_text_judge) driven from C++ through adapter/tsframe_text_judge.hpp
// (pack_text_judge) over small mock types of its own with the shape of TextSLAM's frame, keyframe, mapText and TextFeature.
//
//   text_judge_from_cxx <in.bin> <out.bin>
//     in.bin (tests/test_gpu_text_judge.py): int32 w, h, n, n_dete; the current level-0 image; T_cw of the reference keyframe and of the frame
//     (4x4 row-major doubles); K (fx, fy, cx, cy); detection centres [n_dete][2]; per plane: int32 m, theta[3], box rays [4][2], m x int16 (u, v),
//     m x uint8 featureInten.
//     1. builds the object graph: one reference keyframe (mTcw / mTwc through SetPose, mNcr, vK_scale[0]), the frame (its pyramid through
//        tsframe_set_image, vTextDeteCenter), one mapText per plane with vTextDeteRay and vRefPixs;
//     2. pack_text_judge + one tsframe_text_judge call (cos_min 0, out_margin 6, zncc_min 0.1, with detections: the SearchLocalObjs shape);
//     3. writes Tcr [n][12], reason [n] (int32), pass [n] (uint8), cos [n], zncc [n], box_uv [n][8], dete_bits [n][words] to out.bin.
//   Prints "text judge from C++: ok" and exits 0, 3 without a HIP device, anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tsframe_text_judge.hpp"

namespace mockj {
struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat31 { double v[3]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat33 { double m[9]; double operator()(int r, int c) const { return m[3*r + c]; } double &operator()(int r, int c) { return m[3*r + c]; } };
struct Mat44 { double m[16]; double operator()(int r, int c) const { return m[4*r + c]; } double &operator()(int r, int c) { return m[4*r + c]; } };
struct TextFeature { double u, v, featureInten; };
struct frame {
    Mat44 mTcw, mTwc;
    std::vector<Mat33> vK_scale;
    std::vector<Vec2> vTextDeteCenter;
    void SetPose(const Mat44 &T) {                              // frame.cc: the rigid inverse kept beside mTcw
        mTcw = T;
        for (int i = 0; i < 16; i++) mTwc.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) mTwc(r, c) = T(c, r);
        for (int r = 0; r < 3; r++) mTwc(r, 3) = -(mTwc(r, 0)*T(0, 3) + mTwc(r, 1)*T(1, 3) + mTwc(r, 2)*T(2, 3));
    }
};
struct keyframe : frame { std::vector<Mat31> mNcr; };
struct mapText {
    keyframe *RefKF; int nidx;
    std::vector<Vec2> vTextDeteRay;
    std::vector<TextFeature *> vRefPixs;
    int GetNidx() const { return nidx; }
};
}  // namespace mockj
using namespace mockj;

template <class T> static bool rd(FILE *f, T *p, size_t k) { return k == 0 || fread(p, sizeof(T), k, f) == k; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    int32_t hd[4];
    if (!rd(f, hd, 4)) return 2;
    const int w = hd[0], h = hd[1], n = hd[2], nd = hd[3];
    std::vector<uint8_t> img((size_t)w*h);
    Mat44 Tr, Tc; double K[4];
    if (!rd(f, img.data(), img.size()) || !rd(f, Tr.m, 16) || !rd(f, Tc.m, 16) || !rd(f, K, 4)) return 2;
    keyframe ref; ref.SetPose(Tr);
    Mat33 Km; for (int i = 0; i < 9; i++) Km.m[i] = 0.0;
    Km(0, 0) = K[0]; Km(1, 1) = K[1]; Km(0, 2) = K[2]; Km(1, 2) = K[3]; Km(2, 2) = 1.0;
    ref.vK_scale.push_back(Km);
    frame F; F.SetPose(Tc); F.vK_scale.push_back(Km);
    F.vTextDeteCenter.resize((size_t)nd);
    for (int j = 0; j < nd; j++) if (!rd(f, F.vTextDeteCenter[(size_t)j].v, 2)) return 2;
    std::vector<mapText> texts((size_t)n);
    std::vector<TextFeature> feats;
    std::vector<std::vector<int16_t> > uvs((size_t)n); std::vector<std::vector<uint8_t> > ins((size_t)n);
    ref.mNcr.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        int32_t m; if (!rd(f, &m, 1)) return 2;
        double th[3], ray[8];
        if (!rd(f, th, 3) || !rd(f, ray, 8)) return 2;
        uvs[(size_t)i].resize(2*(size_t)m); ins[(size_t)i].resize((size_t)m);
        if (!rd(f, uvs[(size_t)i].data(), 2*(size_t)m) || !rd(f, ins[(size_t)i].data(), (size_t)m)) return 2;
        for (int k = 0; k < 3; k++) ref.mNcr[(size_t)i](k) = th[k];
        mapText &t = texts[(size_t)i]; t.RefKF = &ref; t.nidx = i;
        t.vTextDeteRay.resize(4);
        for (int b = 0; b < 4; b++) { t.vTextDeteRay[(size_t)b](0) = ray[2*b]; t.vTextDeteRay[(size_t)b](1) = ray[2*b + 1]; }
    }
    fclose(f);
    size_t tot = 0; for (int i = 0; i < n; i++) tot += ins[(size_t)i].size();
    feats.resize(tot);
    size_t at = 0;
    for (int i = 0; i < n; i++)
        for (size_t j = 0; j < ins[(size_t)i].size(); j++, at++) {
            feats[at].u = uvs[(size_t)i][2*j]; feats[at].v = uvs[(size_t)i][2*j + 1]; feats[at].featureInten = ins[(size_t)i][j];
            texts[(size_t)i].vRefPixs.push_back(&feats[at]);
        }
    std::vector<mapText *> objs; for (int i = 0; i < n; i++) objs.push_back(&texts[(size_t)i]);

    void *ctx = nullptr;
    if (tsframe_create(0, &ctx) != TSFRAME_OK) { printf("no HIP device\n"); return 3; }
    if (tsframe_set_image(ctx, img.data(), w, h, 1) != TSFRAME_OK) { fprintf(stderr, "set_image: %s\n", tsframe_last_error(ctx)); return 1; }
    tsframe_adapter::TextJudgePack P;
    if (!tsframe_adapter::pack_text_judge(F, objs, true, P)) { fprintf(stderr, "pack_text_judge failed\n"); return 1; }
    tsframe_adapter::TextJudgeResult R;
    const double Kc[4] = { F.vK_scale[0](0, 0), F.vK_scale[0](1, 1), F.vK_scale[0](0, 2), F.vK_scale[0](1, 2) };
    const int rc = tsframe_adapter::run_text_judge(ctx, 0, P, Kc, 0.0, 6, 0.1, true, R);
    if (rc != TSFRAME_OK) { fprintf(stderr, "tsframe_text_judge (%d): %s\n", rc, tsframe_last_error(ctx)); return 1; }
    for (int i = 0; i < n; i++) {                                 // IdxTextCorDete only for planes that passed
        const std::vector<int> d = R.dete_of(i);
        if (!R.pass[(size_t)i] && !d.empty()) { fprintf(stderr, "plane %d: detections without a pass\n", i); return 1; }
        for (size_t k = 1; k < d.size(); k++) if (d[k] <= d[k - 1]) return 1;
    }
    tsframe_destroy(ctx);
    FILE *o = fopen(argv[2], "wb"); if (!o) { perror(argv[2]); return 2; }
    fwrite(P.Tcr.data(), 8, P.Tcr.size(), o); fwrite(R.reason.data(), 4, R.reason.size(), o); fwrite(R.pass.data(), 1, R.pass.size(), o);
    fwrite(R.cos.data(), 8, R.cos.size(), o); fwrite(R.zncc.data(), 8, R.zncc.size(), o); fwrite(R.box_uv.data(), 8, R.box_uv.size(), o);
    fwrite(R.dete_bits.data(), 4, R.dete_bits.size(), o);
    fclose(o);
    printf("text judge from C++: ok (%d planes, %zu pixels, %d detections)\n", n, tot, nd);
    return 0;
}
