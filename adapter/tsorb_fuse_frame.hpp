// tsorb_fuse_frame.hpp -- header-only body of frame::FeatExtract's steps 3 - 4 (src/frame.cc:229-253: FeatExtracText and tool::BoundFeatDele_T with WinText = -3)
// plus frame::FeatFusion (:257-325) over tsorb_fuse_frame (include/tsorb.h).  The reference extracts the text features detection by detection, tests every one of
// them against two polygons on the host (cv::pointPolygonTest), concatenates scene and text features and grids them (AssignFeaturesToGrid); here ONE call on the
// context that holds the frame (the scene extraction of frame::FeatExtraScene uploaded it) does all of it on the device, returns the fused set and leaves it as
// the set tsorb_match_search / _search_claim / _new_points search: the indices they answer with are indices into vKeys, as everything downstream expects.
// (tsorb_match_set_frame alone would search the scene features only.)  docs/pointpolygon_recalled.md states the polygon test, docs/cvorb_recalled.md the extraction.
// C++11, no OpenCV.  Vec2T is any type with operator()(int) -> double (Eigen's Vec2 in TextSLAM).  Tr is the Traits of adapter/tsorb_text_extract.hpp:
//   typedef ... KeyPoint;  typedef ... Mat;
//   static KeyPoint keypoint(float x, float y, float size, float angle, float response, int octave);
//   static Mat descriptors(const uint8_t *rows, int n);
#ifndef TSORB_FUSE_FRAME_HPP
#define TSORB_FUSE_FRAME_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

// the members of frame that FeatExtract (steps 3 - 4) and FeatFusion fill, under the reference's names; IdxNewText is FeatExtract's local of that name
template <class Tr> struct FusedFrame {
    std::vector<typename Tr::KeyPoint> vKeysScene; typename Tr::Mat mDescrScene;
    std::vector<std::vector<typename Tr::KeyPoint> > vKeysText; std::vector<typename Tr::Mat> mDescrText;
    std::vector<typename Tr::KeyPoint> vKeys; typename Tr::Mat mDescr;
    std::vector<int> vTextObjInfo; std::vector<size_t> vKeysSceneIdx; std::vector<std::vector<size_t> > vKeysTextIdx;
    std::vector<std::vector<int> > IdxNewText;
    int iNScene, iNTextObj, iNTextFea, iN;
    FusedFrame() : iNScene(0), iNTextObj(0), iNTextFea(0), iN(0) {}
};

// ctx: the tsorb context whose resident batch holds the frame (ExtractorCore::tsorb_context()), frame: its index in that batch (0 for the per-frame call);
// TextDete, vTextDeteMin, vTextDeteMax: the frame's members of those names; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY; scene_room: the room the first
// attempt leaves for scene rows (the reference's extractor returns about 1000).  Returns TSORB_OK or the error of tsorb_fuse_frame (out is then empty).  A capacity
// that was too small: once more with the counts the call reported, which always suffice.
template <class Tr, class Vec2T>
int feat_extract_fuse(void *ctx, int frame, const std::vector<std::vector<Vec2T> > &TextDete, const std::vector<Vec2T> &vTextDeteMin, const std::vector<Vec2T> &vTextDeteMax,
                      const double bounds[4], FusedFrame<Tr> &out, int nfeatures = 500, double win = -3.0, int scene_room = 2048) {
    out = FusedFrame<Tr>();
    out.mDescrScene = Tr::descriptors(0, 0); out.mDescr = Tr::descriptors(0, 0);
    const size_t nd = TextDete.size();
    if (vTextDeteMin.size() != nd || vTextDeteMax.size() != nd || scene_room < 1) return TSORB_ERR_ARG;
    std::vector<double> quad(8*nd), bbox(4*nd);
    for (size_t i = 0; i < nd; i++) {
        if (TextDete[i].size() != 4) return TSORB_ERR_ARG;                  // a detection is four corners (tool::GetNewDeteBox reads [0] .. [3])
        for (int k = 0; k < 4; k++) { quad[8*i + 2*k] = TextDete[i][k](0); quad[8*i + 2*k + 1] = TextDete[i][k](1); }
        bbox[4*i] = vTextDeteMin[i](0); bbox[4*i + 1] = vTextDeteMin[i](1); bbox[4*i + 2] = vTextDeteMax[i](0); bbox[4*i + 3] = vTextDeteMax[i](1);
    }
    int cap_text = nfeatures + 64;                                          // the quota plus room for the ties a cut keeps
    long cap = (long)scene_room + (long)nd*cap_text;
    std::vector<float> kp; std::vector<uint8_t> desc; std::vector<int32_t> obj, src, off(nd + 1, 0), raw(nd, 0); int32_t n_out[2] = { 0, 0 };
    int rc = TSORB_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (cap > 0x7fffffffL/32) return TSORB_ERR_ARG;
        kp.assign(6*(size_t)cap, 0.f); desc.assign(32*(size_t)cap, 0); obj.assign((size_t)cap, 0); src.assign((size_t)cap, 0);
        n_out[0] = n_out[1] = -1;
        rc = tsorb_fuse_frame(ctx, frame, (int)nd, nd ? quad.data() : 0, nd ? bbox.data() : 0, win, nfeatures, cap_text, (int)cap, bounds[0], bounds[1], bounds[2], bounds[3],
                              kp.data(), desc.data(), obj.data(), src.data(), off.data(), nd ? raw.data() : 0, n_out);
        if (rc != TSORB_ERR_ARG || n_out[0] < 0) break;                     // done, or an error that reported no counts
        int most = 0; long sum = 0;
        for (size_t i = 0; i < nd; i++) { if (raw[i] > most) most = raw[i]; sum += raw[i]; }
        if (most <= cap_text && n_out[1] <= cap) break;
        if (most > cap_text) cap_text = most;                               // (then n counted only the detections that fit: room for every raw row)
        cap = (long)n_out[0] + sum;
        if (cap < 1) cap = 1;
    }
    if (rc != TSORB_OK) return rc;
    const int ns = n_out[0], n = n_out[1];
    out.iNScene = ns; out.iNTextObj = (int)nd; out.iNTextFea = n - ns; out.iN = n;
    out.vKeys.reserve((size_t)n);
    for (int j = 0; j < n; j++) { const float *k = kp.data() + 6*(size_t)j; out.vKeys.push_back(Tr::keypoint(k[0], k[1], k[2], k[3], k[4], (int)k[5])); }
    out.mDescr = Tr::descriptors(desc.data(), n);
    out.vTextObjInfo.assign(obj.begin(), obj.begin() + n);
    out.vKeysScene.assign(out.vKeys.begin(), out.vKeys.begin() + ns);
    out.mDescrScene = Tr::descriptors(desc.data(), ns);
    out.vKeysSceneIdx.resize((size_t)ns);
    for (int j = 0; j < ns; j++) out.vKeysSceneIdx[(size_t)j] = (size_t)j;
    out.vKeysText.resize(nd); out.mDescrText.resize(nd); out.vKeysTextIdx.resize(nd); out.IdxNewText.resize(nd);
    for (size_t i = 0; i < nd; i++) {
        const int a = off[i], b = off[i + 1];
        out.vKeysText[i].assign(out.vKeys.begin() + a, out.vKeys.begin() + b);
        out.mDescrText[i] = Tr::descriptors(desc.data() + 32*(size_t)a, b - a);
        for (int j = a; j < b; j++) { out.vKeysTextIdx[i].push_back((size_t)j); out.IdxNewText[i].push_back(src[(size_t)j]); }
    }
    return TSORB_OK;
}

}  // namespace tsorb_adapter
#endif
