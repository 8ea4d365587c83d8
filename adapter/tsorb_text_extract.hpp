// tsorb_text_extract.hpp -- header-only body of frame::FeatExtracText (src/frame.cc:334-355) over tsorb_text_extract (include/tsorb.h): the reference
// builds a masked copy of the frame per text detection (tool::GetMask) and runs cv::ORB::create()->detect on it and ->compute on the frame, one
// detection after the other; here the quads of all detections go to ONE call on the context that already holds the frame (the scene extraction of
// frame::FeatExtraScene uploaded it), and the result is split again.  The detections are independent of each other, so the result is the same as the
// loop's (docs/cvorb_recalled.md states the arithmetic and its two deliberate differences from OpenCV: ties at a cut, order inside a level).
// C++11, no OpenCV.  Vec2T is any type with operator()(int) -> double (Eigen's Vec2 in TextSLAM).  Tr names the output types:
//   typedef ... KeyPoint;  typedef ... Mat;
//   static KeyPoint keypoint(float x, float y, float size, float angle, float response, int octave);   // cv::KeyPoint(x, y, size, angle, response, octave)
//   static Mat descriptors(const uint8_t *rows, int n);                                                // cv::Mat(n, 32, CV_8U, (void *)rows).clone(); n == 0: cv::Mat()
// (over the real types these two lines are the whole Traits; tests/cxx/text_orb_from_cxx.cpp has them over mock types.)
// These are the RAW text features.  The -3-px boundary test of frame.cc:244 (tool::BoundFeatDele_T) and frame::FeatFusion run on the device in
// tsorb_fuse_frame (adapter/tsorb_fuse_frame.hpp), which makes this extraction part of its own call; a caller of this header alone keeps both on the host.
#ifndef TSORB_TEXT_EXTRACT_HPP
#define TSORB_TEXT_EXTRACT_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

// ctx: the tsorb context whose resident batch holds the frame (ExtractorCore::tsorb_context()), frame: its index in that batch (0 for the per-frame call).
// KeysTextRaw[i], DescripTextRaw[i]: the text features of TextDete[i] (a detection without a keypoint: an empty vector and Tr::descriptors(.., 0)).
// Returns TSORB_OK or the error of tsorb_text_extract (the outputs then have one empty entry per detection).
template <class Tr, class Vec2T>
int feat_extrac_text(void *ctx, int frame, const std::vector<std::vector<Vec2T> > &TextDete, std::vector<std::vector<typename Tr::KeyPoint> > &KeysTextRaw,
                     std::vector<typename Tr::Mat> &DescripTextRaw, int nfeatures = 500) {
    const size_t n = TextDete.size();
    KeysTextRaw.assign(n, std::vector<typename Tr::KeyPoint>());
    DescripTextRaw.assign(n, Tr::descriptors(0, 0));
    if (n == 0) return TSORB_OK;
    std::vector<double> quad(8*n);
    for (size_t i = 0; i < n; i++) {
        if (TextDete[i].size() != 4) return TSORB_ERR_ARG;                  // a detection is four corners (tool::GetMask reads [0] .. [3])
        for (int k = 0; k < 4; k++) { quad[8*i + 2*k] = TextDete[i][k](0); quad[8*i + 2*k + 1] = TextDete[i][k](1); }
    }
    int cap = nfeatures + 64;                                               // the quota plus room for the ties a cut keeps
    std::vector<float> kp; std::vector<uint8_t> desc; std::vector<int32_t> cnt(n, 0);
    int rc = TSORB_OK;
    for (int attempt = 0; attempt < 2; attempt++) {                         // a detection with more ties than that: once more with the largest count
        kp.assign(6*n*(size_t)cap, 0.f); desc.assign(32*n*(size_t)cap, 0);
        rc = tsorb_text_extract(ctx, frame, (int)n, quad.data(), nfeatures, cap, kp.data(), desc.data(), cnt.data());
        int most = 0;
        for (size_t i = 0; i < n; i++) if (cnt[i] > most) most = cnt[i];
        if (rc != TSORB_ERR_ARG || most <= cap) break;
        cap = most;
    }
    if (rc != TSORB_OK) return rc;
    for (size_t i = 0; i < n; i++) {
        const float *k = kp.data() + 6*i*(size_t)cap;
        KeysTextRaw[i].reserve((size_t)cnt[i]);
        for (int j = 0; j < cnt[i]; j++) KeysTextRaw[i].push_back(Tr::keypoint(k[6*j], k[6*j + 1], k[6*j + 2], k[6*j + 3], k[6*j + 4], (int)k[6*j + 5]));
        DescripTextRaw[i] = Tr::descriptors(desc.data() + 32*i*(size_t)cap, cnt[i]);
    }
    return TSORB_OK;
}

}  // namespace tsorb_adapter
#endif
