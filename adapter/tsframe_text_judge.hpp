// tsframe_text_judge.hpp -- header-only gather for tsframe_text_judge (include/tsframe.h): tracking::TextJudgeSingle for a set of planes in one call.
// Templated over the object types, so the same code is compiled against TextSLAM's types (frame, keyframe, mapText, TextFeature) and against the
// mock types of tests/cxx/text_judge_from_cxx.cpp.  What it touches (src/frame.h, src/keyframe.h, src/mapText.h):
//   F.mTcw (Mat44, (r, c)), F.vTextDeteCenter (vector<Vec2>, (i)),
//   obj->RefKF->mNcr[obj->GetNidx()] (Mat31, (i)), obj->RefKF->mTwc (Mat44: the inverse of mTcw that SetPose keeps), obj->RefKF->vK_scale[0]
//   (Mat33, (r, c)), obj->vTextDeteRay (vector<Vec2>, 4 corners), obj->vRefPixs (vector<TextFeature *>: u, v, featureInten).
// Tcr = F.mTcw * RefKF->mTwc, the top three rows, summed k = 0..3 as Eigen's 4x4 product.  The reference writes mTcw.inverse() (a general 4x4
// inverse): the same matrix up to the last bits of the rigid inverse SetPose stores.
#ifndef TSFRAME_TEXT_JUDGE_HPP
#define TSFRAME_TEXT_JUDGE_HPP
#include <stdint.h>
#include <cmath>
#include <vector>
#include "tsframe.h"

namespace tsframe_adapter {

struct TextJudgePack {
    int n;
    std::vector<double> theta, Tcr, box_ray, dete_xy;          // [n][3], [n][12], [n][8], [n_dete][2]
    std::vector<int32_t> pix_off;                               // [n + 1]
    std::vector<int16_t> pix_uv;                                // [m][2]
    std::vector<uint8_t> pix_inten;                             // [m]
    double K_ref[4];                                            // fx, fy, cx, cy of the reference keyframes' level 0
    TextJudgePack() : n(0) { K_ref[0] = K_ref[1] = K_ref[2] = K_ref[3] = 0.0; }
};

struct TextJudgeResult {
    std::vector<uint8_t> pass; std::vector<int32_t> reason; std::vector<double> cos, zncc, box_uv; std::vector<uint32_t> dete_bits;
    int words;
    TextJudgeResult() : words(0) {}
    // tracking.cc:2116-2128: IdxTextCorDete of plane i, detections in increasing order
    std::vector<int> dete_of(int i) const {
        std::vector<int> out;
        for (int w = 0; w < words; w++)
            for (int b = 0; b < 32; b++) if ((dete_bits[(size_t)i*words + w] >> b) & 1u) out.push_back(32*w + b);
        return out;
    }
};

// Gathers the planes objs[0 .. n) of the current frame F.  with_dete: also F.vTextDeteCenter (the 5-argument overload, SearchLocalObjs).
// Returns false if a plane has no 4-corner box, a reference pixel does not fit int16 / uint8, or the reference keyframes disagree on K.
template <class Frame, class MapText>
bool pack_text_judge(const Frame &F, const std::vector<MapText *> &objs, bool with_dete, TextJudgePack &P) {
    const size_t n = objs.size();
    P.n = (int)n;
    P.theta.assign(3*n, 0.0); P.Tcr.assign(12*n, 0.0); P.box_ray.assign(8*n, 0.0);
    P.pix_off.assign(n + 1, 0); P.pix_uv.clear(); P.pix_inten.clear(); P.dete_xy.clear();
    for (size_t i = 0; i < n; i++) {
        MapText *obj = objs[i];
        const int nidx = obj->GetNidx();
        for (int k = 0; k < 3; k++) P.theta[3*i + k] = obj->RefKF->mNcr[(size_t)nidx](k);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++)
                P.Tcr[12*i + 4*r + c] = F.mTcw(r, 0)*obj->RefKF->mTwc(0, c) + F.mTcw(r, 1)*obj->RefKF->mTwc(1, c) + F.mTcw(r, 2)*obj->RefKF->mTwc(2, c)
                                        + F.mTcw(r, 3)*obj->RefKF->mTwc(3, c);
        if (obj->vTextDeteRay.size() != 4) return false;
        for (int b = 0; b < 4; b++) { P.box_ray[8*i + 2*b] = obj->vTextDeteRay[(size_t)b](0); P.box_ray[8*i + 2*b + 1] = obj->vTextDeteRay[(size_t)b](1); }
        const double K[4] = { obj->RefKF->vK_scale[0](0, 0), obj->RefKF->vK_scale[0](1, 1), obj->RefKF->vK_scale[0](0, 2), obj->RefKF->vK_scale[0](1, 2) };
        for (int k = 0; k < 4; k++) {
            if (i == 0) P.K_ref[k] = K[k];
            else if (P.K_ref[k] != K[k]) return false;
        }
        for (size_t j = 0; j < obj->vRefPixs.size(); j++) {
            const double u = obj->vRefPixs[j]->u, v = obj->vRefPixs[j]->v, I = obj->vRefPixs[j]->featureInten;
            if (!(u >= -32768.0 && u <= 32767.0 && v >= -32768.0 && v <= 32767.0 && I >= 0.0 && I <= 255.0)) return false;
            if (u != std::floor(u) || v != std::floor(v) || I != std::floor(I)) return false;    // GetBoxAllPixs: integer pixels, 8-bit intensities
            P.pix_uv.push_back((int16_t)u); P.pix_uv.push_back((int16_t)v); P.pix_inten.push_back((uint8_t)I);
        }
        P.pix_off[i + 1] = (int32_t)(P.pix_inten.size());
    }
    if (with_dete)
        for (size_t j = 0; j < F.vTextDeteCenter.size(); j++) { P.dete_xy.push_back(F.vTextDeteCenter[j](0)); P.dete_xy.push_back(F.vTextDeteCenter[j](1)); }
    return true;
}

// One tsframe_text_judge call on the frame's resident pyramid (ctx), thresholds as the call site passes them (cos_min 0 = the reference).
inline int run_text_judge(void *ctx, int level, const TextJudgePack &P, const double K[4], double cos_min, int out_margin, double zncc_min,
                          bool with_dete, TextJudgeResult &R) {
    const size_t n = (size_t)P.n;
    const int n_dete = with_dete ? (int)(P.dete_xy.size()/2) : 0;
    R.words = with_dete ? (n_dete + 31)/32 : 0;
    R.pass.assign(n, 0); R.reason.assign(n, 0); R.cos.assign(n, 0.0); R.zncc.assign(n, 0.0); R.box_uv.assign(8*n, 0.0);
    R.dete_bits.assign(n*(size_t)R.words, 0u);
    if (n == 0) return TSFRAME_OK;
    return tsframe_text_judge(ctx, level, P.n, P.theta.data(), P.Tcr.data(), P.box_ray.data(), P.pix_off.data(),
                              P.pix_uv.empty() ? nullptr : P.pix_uv.data(), P.pix_inten.empty() ? nullptr : P.pix_inten.data(), P.K_ref, K,
                              cos_min, out_margin, zncc_min, n_dete, n_dete ? P.dete_xy.data() : nullptr,
                              R.pass.data(), R.reason.data(), R.cos.data(), R.zncc.data(), R.box_uv.data(), with_dete ? R.dete_bits.data() : nullptr);
}

}  // namespace tsframe_adapter
#endif
