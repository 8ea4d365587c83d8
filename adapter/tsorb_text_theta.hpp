// tsorb_text_theta.hpp -- the planes of new text detections through ONE tsorb_match_text_theta_ransac call (include/tsorb.h): the bodies of
// tracking::InitialTextObjs (src/tracking.cc:1631-1661, with GetTextTheta :1664-1734 and SolveTheta :1870-1917) and of the two-view initializer's
// initializer::InitialTextObjs (src/initializer.cc:111-183, with CalculateTextTheta :1004-1061).  Header-only, C++11, no OpenCV or Eigen: the templates reach the
// reference's objects through the member names the reference uses, so they compile against the real types inside the TextSLAM tree and against plain structs of
// the same shape (tests/cxx/text_theta_from_cxx.cpp).  docs/texttheta_recalled.md states the arithmetic the call runs.
//
// What each function restates:
//   draw_theta_triples       tool::GetRANSACIdx             src/tool.cc:1366-1390       the available list refilled for EVERY hypothesis (Sim3Solver's is not)
//   initial_text_objs        tracking::InitialTextObjs      src/tracking.cc:1631-1661   rho by triangulation on the device, 200 triples per detection
//   initial_text_objs_init   initializer::InitialTextObjs   src/initializer.cc:111-183  rho = TextKeys3D[i][j](2), mMaxIterations triples per detection
//
// Traits (adapter/textslam_traits.hpp has them over the real types):
//   int  random_int(int lo, int hi)     DUtils::Random::RandomInt(lo, hi): uniform in [lo, hi].  The reference draws a detection's triples right before it scores
//                                       them and nothing else draws in between: drawing every detection's triples, detection by detection in loop order, before the
//                                       one call leaves every draw what it was.
//   void seed_rand_once()               DUtils::Random::SeedRandOnce(0), where the reference calls it (tool.cc:1375, initializer.cc:130)
//   void tcr_of(Tcw, Trw, double[12])   the top three rows of Tcw * Trw.inverse(), the reference's own expression (tracking.cc:1667, initializer.cc:1013)
//   Mat31 vec3(double, double, double)
#ifndef TSORB_TEXT_THETA_HPP
#define TSORB_TEXT_THETA_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

// H triples over n features (n >= 3), appended to `triple`: vAvailableIndices = InitialVec(n) per hypothesis; randi = RandomInt(0, size - 1), idx = avail[randi],
// avail[randi] = avail.back(), pop_back
template <class T>
inline void draw_theta_triples(int n, int H, std::vector<int32_t> &triple) {
    std::vector<int32_t> avail;
    for (int h = 0; h < H; h++) {
        avail.resize((size_t)n);
        for (int i = 0; i < n; i++) avail[(size_t)i] = i;
        for (int j = 0; j < 3; j++) {
            const int randi = T::random_int(0, (int)avail.size() - 1);
            triple.push_back(avail[(size_t)randi]);
            avail[(size_t)randi] = avail.back(); avail.pop_back();
        }
    }
}

// what one call takes and gives; plane k is detection det[k]
struct TextThetaCall {
    std::vector<int32_t> det, off, hyp_off, triple, sel;
    std::vector<float> host_xy, targ_xy, p3d;
    std::vector<double> rho, theta, score, rho_out;
    double Tcr[12], K[4];
    bool rho_given;
    int rc;
    TextThetaCall() : rho_given(false), rc(0) { off.push_back(0); hyp_off.push_back(0); for (int i = 0; i < 12; i++) Tcr[i] = 0.0; for (int i = 0; i < 4; i++) K[i] = 0.0; }
    int n_plane() const { return (int)det.size(); }
    void close_plane(int i0) { det.push_back((int32_t)i0); off.push_back((int32_t)(host_xy.size()/2)); hyp_off.push_back((int32_t)(triple.size()/3)); }
    int run(void *orbCtx) {
        const size_t P = det.size(), N = host_xy.size()/2;
        sel.assign(P, -1); theta.assign(3*P, 0.0); score.assign(P, 0.0); p3d.assign(3*N, 0.f); rho_out.assign(N, 0.0);
        rc = tsorb_match_text_theta_ransac(orbCtx, (int)P, off.data(), N ? host_xy.data() : 0, N ? targ_xy.data() : 0, rho_given && N ? rho.data() : 0, Tcr, K, hyp_off.data(),
                                           triple.empty() ? 0 : triple.data(), P ? sel.data() : 0, P ? theta.data() : 0, P ? score.data() : 0, N ? p3d.data() : 0,
                                           N ? rho_out.data() : 0, 0, 0);
        return rc;
    }
};

// mNcr[i0] = theta, vNGOOD[i0] = true for every plane that kept a hypothesis (tracking.cc:1658-1659, initializer.cc:179-180)
template <class T, class KF>
inline void scatter_text_theta(const TextThetaCall &c, KF *kf) {
    for (size_t k = 0; k < c.det.size(); k++) {
        if (c.sel[k] < 0) continue;
        const size_t i0 = (size_t)c.det[k];
        kf->mNcr[i0] = T::vec3(c.theta[3*k], c.theta[3*k + 1], c.theta[3*k + 2]);
        kf->vNGOOD[i0] = true;
    }
}

// The body of tracking::InitialTextObjs in three steps: gather_text_objs (the NaN / false pushes, the detections the loop reaches, Tcr, K, the draws), the call,
// scatter_text_theta.  lastKF: cfLastKeyframe (vTextDeteCorMap, vKeysNewTextTrack, mTcw, iNTextObj, mNcr, vNGOOD); cur: cfCurrentFrame (vKeysTextTrack, mTcw, mK).
// initial_text_objs returns TSORB_OK or the call's error: mNcr / vNGOOD then keep the NaN / false every detection starts with.
template <class T, class KF, class Frame>
inline void gather_text_objs(KF *lastKF, const Frame &cur, TextThetaCall &c, int iMaxIterations = 200, size_t thresh_textnum = 8) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t j0 = 0; j0 < (size_t)lastKF->iNTextObj; j0++) { lastKF->mNcr.push_back(T::vec3(nan, nan, nan)); lastKF->vNGOOD.push_back(false); }     // :1636-1639
    c = TextThetaCall();
    T::tcr_of(cur.mTcw, lastKF->mTcw, c.Tcr);                                                                          // GetTextTheta(..., cfLastKeyframe->mTcw, cfCurrentFrame.mTcw, ...)
    c.K[0] = cur.mK(0, 0); c.K[1] = cur.mK(1, 1); c.K[2] = cur.mK(0, 2); c.K[3] = cur.mK(1, 2);
    for (size_t i0 = 0; i0 < lastKF->vTextDeteCorMap.size(); i0++) {
        if (lastKF->vTextDeteCorMap[i0] >= 0) continue;
        const size_t n = lastKF->vKeysNewTextTrack[i0].size();
        if (n < thresh_textnum) continue;
        for (size_t j = 0; j < n; j++) {
            c.host_xy.push_back(lastKF->vKeysNewTextTrack[i0][j].x); c.host_xy.push_back(lastKF->vKeysNewTextTrack[i0][j].y);
            c.targ_xy.push_back(cur.vKeysTextTrack[i0][j].x); c.targ_xy.push_back(cur.vKeysTextTrack[i0][j].y);
        }
        if (n >= 3) { T::seed_rand_once(); draw_theta_triples<T>((int)n, iMaxIterations, c.triple); }                 // GetRANSACIdx: false below 3 features, nothing drawn
        c.close_plane((int)i0);
    }
}
template <class T, class KF, class Frame>
inline int initial_text_objs(void *orbCtx, KF *lastKF, const Frame &cur, TextThetaCall *keep = 0, int iMaxIterations = 200, size_t thresh_textnum = 8) {
    TextThetaCall c;
    gather_text_objs<T>(lastKF, cur, c, iMaxIterations, thresh_textnum);
    const int rc = c.run(orbCtx);                                                                                      // ONE call for every detection
    if (rc == TSORB_OK) scatter_text_theta<T>(c, lastKF);
    if (keep) *keep = c;
    return rc;
}

// The body of initializer::InitialTextObjs.  TextKeys1 / TextKeys2 [i][j]: the feature's keypoint in F1 / F2 as tracking::InitialLandmarker builds them (Vec2 of the
// floats pt.x, pt.y); TextKeys3D [i][j](2) = rho = 1.0/IniP3D[.].z (its (0), (1) are the rays the call forms again from TextKeys1 by the same expression).
// K = F1->fx, fy, cx, cy.  A plane of fewer than 4 features draws nothing: one of exactly 3 keeps the reference's all-zero triples, one below 3 is skipped.
template <class T, class KF, class Keys2, class Keys3>
inline void gather_text_objs_init(KF *F1, const KF *F2, const std::vector<std::vector<Keys2> > &TextKeys1, const std::vector<std::vector<Keys3> > &TextKeys3D,
                                  const std::vector<std::vector<Keys2> > &TextKeys2, int mMaxIterations, TextThetaCall &c, size_t thresh_textnum = 4) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t j0 = 0; j0 < (size_t)F1->iNTextObj; j0++) { F1->mNcr.push_back(T::vec3(nan, nan, nan)); F1->vNGOOD.push_back(false); }                   // :115-118
    c = TextThetaCall(); c.rho_given = true;
    T::tcr_of(F2->mTcw, F1->mTcw, c.Tcr);                                                                              // T21 = F2->mTcw * F1->mTcw.inverse(), :1013
    c.K[0] = F1->fx; c.K[1] = F1->fy; c.K[2] = F1->cx; c.K[3] = F1->cy;
    T::seed_rand_once();                                                                                               // :130
    for (size_t i1 = 0; i1 < TextKeys3D.size(); i1++) {
        const size_t n = TextKeys3D[i1].size();
        for (size_t j = 0; j < n; j++) {
            c.host_xy.push_back((float)TextKeys1[i1][j](0)); c.host_xy.push_back((float)TextKeys1[i1][j](1));
            c.targ_xy.push_back((float)TextKeys2[i1][j](0)); c.targ_xy.push_back((float)TextKeys2[i1][j](1));
            c.rho.push_back(TextKeys3D[i1][j](2));
        }
        if (n >= thresh_textnum) draw_theta_triples<T>((int)n, mMaxIterations, c.triple);                              // :134-148
        else if (n >= 3) c.triple.insert(c.triple.end(), 3*(size_t)mMaxIterations, 0);                                 // RansacIdxCell stays (0, 0, 0); :156 skips n < 3
        c.close_plane((int)i1);
    }
}
template <class T, class KF, class Keys2, class Keys3>
inline int initial_text_objs_init(void *orbCtx, KF *F1, const KF *F2, const std::vector<std::vector<Keys2> > &TextKeys1, const std::vector<std::vector<Keys3> > &TextKeys3D,
                                  const std::vector<std::vector<Keys2> > &TextKeys2, int mMaxIterations, TextThetaCall *keep = 0, size_t thresh_textnum = 4) {
    TextThetaCall c;
    gather_text_objs_init<T>(F1, F2, TextKeys1, TextKeys3D, TextKeys2, mMaxIterations, c, thresh_textnum);
    const int rc = c.run(orbCtx);                                                                                      // ONE call for every detection
    if (rc == TSORB_OK) scatter_text_theta<T>(c, F1);
    if (keep) *keep = c;
    return rc;
}

}  // namespace tsorb_adapter
#endif
