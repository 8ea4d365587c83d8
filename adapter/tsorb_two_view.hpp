// tsorb_two_view.hpp -- header-only replacement of initializer::FindHomography + FindFundamental (src/initializer.cc:91-96, :185-284) over
// tsorb_match_two_view_ransac (include/tsorb.h): the 2 x 200 eight-point fits and their scoring over all matches that tracking::Initialization runs on every frame
// until a pair initialises.  C++11, no OpenCV, no Eigen outside the traits.  docs/twoview_recalled.md states the arithmetic; what runs between the gather and the
// outputs -- the fits, the scoring, the two keep loops -- is what the library does.  Subset drawing (DUtils::Random, :68-88) stays with the reference.
// The templates reach the reference's objects through the member names the reference uses: keys[i].pt.x / .y (cv::KeyPoint), matches12[i].first / .second
// (initializer::Match), sets[it][j] (mvSets).  Tr gives the 3 x 3 float matrix type:
//   typedef ... Mat33f;                                         // cv::Mat in the reference
//   static void assign33(Mat33f &M, const float m[9]);          // M = the row-major 3 x 3, CV_32F
// e.g. struct CvTwoViewTraits { typedef cv::Mat Mat33f; static void assign33(cv::Mat &M, const float m[9]) { cv::Mat(3, 3, CV_32F, (void *)m).copyTo(M); } };
#ifndef TSORB_TWO_VIEW_HPP
#define TSORB_TWO_VIEW_HPP
#include <stdint.h>
#include <cmath>
#include <cstddef>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

// initializer::Normalize's statistics (:821-852) over ALL keypoints of a frame, its float loops restated: norm = meanX, meanY, sX, sY.  (The normalised points and T
// are formed by the library from these four floats.)  Build the including file without floating-point contraction and without -ffast-math, as the reference is.
template <class Keys>
inline void two_view_normalize(const Keys &vKeys, float norm[4]) {
    float meanX = 0, meanY = 0;
    const int N = (int)vKeys.size();
    for (int i = 0; i < N; i++) { meanX += vKeys[(size_t)i].pt.x; meanY += vKeys[(size_t)i].pt.y; }
    meanX = meanX/N; meanY = meanY/N;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < N; i++) {
        const float dx = vKeys[(size_t)i].pt.x - meanX, dy = vKeys[(size_t)i].pt.y - meanY;
        meanDevX += std::fabs(dx); meanDevY += std::fabs(dy);
    }
    meanDevX = meanDevX/N; meanDevY = meanDevY/N;
    const float sX = 1.0/meanDevX, sY = 1.0/meanDevY;
    norm[0] = meanX; norm[1] = meanY; norm[2] = sX; norm[3] = sY;
}

// What one Initialize sends and receives
struct TwoViewCall {
    std::vector<float> xy1, xy2; std::vector<int32_t> subset; std::vector<uint8_t> inlier_h, inlier_f;
    float norm1[4], norm2[4], H21[9], F21[9], score[2]; int32_t sel[2];
    int n() const { return (int)(xy1.size()/2); }
    int n_hyp() const { return (int)(subset.size()/8); }
};

// the matched pixels (CheckHomography's kp1 = mvKeys1[mvMatches12[i].first], kp2 = mvKeys2[mvMatches12[i].second]) and mvSets as [n_hyp][8]
template <class Keys, class Matches, class Sets>
inline void two_view_gather(const Keys &vKeys1, const Keys &vKeys2, const Matches &vMatches12, const Sets &vSets, TwoViewCall &c) {
    c.xy1.clear(); c.xy2.clear(); c.subset.clear();
    for (size_t i = 0; i < vMatches12.size(); i++) {
        const size_t i1 = (size_t)vMatches12[i].first, i2 = (size_t)vMatches12[i].second;
        c.xy1.push_back(vKeys1[i1].pt.x); c.xy1.push_back(vKeys1[i1].pt.y);
        c.xy2.push_back(vKeys2[i2].pt.x); c.xy2.push_back(vKeys2[i2].pt.y);
    }
    for (size_t it = 0; it < vSets.size(); it++) for (size_t j = 0; j < 8; j++) c.subset.push_back((int32_t)vSets[it][j]);
}

// the reference's outputs from the call's: vbMatchesInliers, score, and the kept matrix (left as it was when nothing was kept, as the reference leaves its empty Mat)
template <class Tr>
inline bool two_view_fill(const TwoViewCall &c, std::vector<bool> &vbMatchesInliersH, float &SH, typename Tr::Mat33f &H,
                          std::vector<bool> &vbMatchesInliersF, float &SF, typename Tr::Mat33f &F) {
    const size_t n = (size_t)c.n();
    vbMatchesInliersH.assign(n, false); vbMatchesInliersF.assign(n, false);
    for (size_t i = 0; i < n; i++) { vbMatchesInliersH[i] = c.inlier_h[i] != 0; vbMatchesInliersF[i] = c.inlier_f[i] != 0; }
    SH = c.score[0]; SF = c.score[1];
    if (c.sel[0] >= 0) Tr::assign33(H, c.H21);
    if (c.sel[1] >= 0) Tr::assign33(F, c.F21);
    return c.sel[0] >= 0 && c.sel[1] >= 0;
}

// FindHomography(vbMatchesInliersH, SH, H); FindFundamental(vbMatchesInliersF, SF, F); in ONE call.  norm1: frame 1's Normalize statistics when the caller keeps them
// (they do not change while the initializer's reference frame stays), NULL = computed here.  Returns false on a device or argument error (the outputs are untouched;
// tsorb_last_error(orbCtx) says what) and when either model kept no hypothesis: the reference would hand an empty cv::Mat to ReconstructH / ReconstructF, the caller
// returns false from Initialize instead.
template <class Tr, class Keys, class Matches, class Sets>
inline bool find_h_and_f(void *orbCtx, const Keys &vKeys1, const Keys &vKeys2, const Matches &vMatches12, const Sets &vSets, float sigma,
                         std::vector<bool> &vbMatchesInliersH, float &SH, typename Tr::Mat33f &H, std::vector<bool> &vbMatchesInliersF, float &SF, typename Tr::Mat33f &F,
                         const float *norm1 = 0, TwoViewCall *keep = 0) {
    TwoViewCall local, &c = keep ? *keep : local;
    two_view_gather(vKeys1, vKeys2, vMatches12, vSets, c);
    if (norm1) for (int i = 0; i < 4; i++) c.norm1[i] = norm1[i]; else two_view_normalize(vKeys1, c.norm1);
    two_view_normalize(vKeys2, c.norm2);
    const size_t n = (size_t)c.n();
    c.inlier_h.assign(n ? n : 1, 0); c.inlier_f.assign(n ? n : 1, 0);
    const int rc = tsorb_match_two_view_ransac(orbCtx, (int)n, c.xy1.data(), c.xy2.data(), c.norm1, c.norm2, c.n_hyp(), c.subset.data(), sigma,
                                               c.inlier_h.data(), c.inlier_f.data(), c.H21, c.F21, c.score, c.sel, 0, 0);
    if (rc != TSORB_OK) return false;
    return two_view_fill<Tr>(c, vbMatchesInliersH, SH, H, vbMatchesInliersF, SF, F);
}

// ---- ReconstructH / ReconstructF (src/initializer.cc:98-105, :531-802, CheckRT :868-977) over tsorb_match_two_view_reconstruct; docs/twoview_reconstruct_recalled.md
// states the arithmetic.  On top of the members above, Tr gives
//   static float at33(const Mat33f &M, int r, int c);           // M.at<float>(r, c)
//   typedef ... Mat31f;                                         // cv::Mat in the reference
//   static void assign31(Mat31f &t, const float v[3]);          // t = the 3 x 1, CV_32F
// and vP3D's elements have the members x, y, z (cv::Point3f).

// What one reconstruction sends and receives
struct ReconstructCall {
    std::vector<float> xy1, xy2, p3d; std::vector<uint8_t> inlier, triangulated;
    float M21[9], K[4], R21[9], t21[3]; int32_t result[6];
    int n() const { return (int)(xy1.size()/2); }
};

// the matched pixels as above, vbMatchesInliers as bytes, and the floats of the model and of mK (fx, fy, cx, cy)
template <class Tr, class Keys, class Matches>
inline void reconstruct_gather(const Keys &vKeys1, const Keys &vKeys2, const Matches &vMatches12, const std::vector<bool> &vbMatchesInliers,
                               const typename Tr::Mat33f &M21, const typename Tr::Mat33f &K, ReconstructCall &c) {
    c.xy1.clear(); c.xy2.clear(); c.inlier.clear();
    for (size_t i = 0; i < vMatches12.size(); i++) {
        const size_t i1 = (size_t)vMatches12[i].first, i2 = (size_t)vMatches12[i].second;
        c.xy1.push_back(vKeys1[i1].pt.x); c.xy1.push_back(vKeys1[i1].pt.y);
        c.xy2.push_back(vKeys2[i2].pt.x); c.xy2.push_back(vKeys2[i2].pt.y);
        c.inlier.push_back(i < vbMatchesInliers.size() && vbMatchesInliers[i] ? 1 : 0);
    }
    for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) c.M21[3*r + k] = Tr::at33(M21, r, k);
    c.K[0] = Tr::at33(K, 0, 0); c.K[1] = Tr::at33(K, 1, 1); c.K[2] = Tr::at33(K, 0, 2); c.K[3] = Tr::at33(K, 1, 2);
}

// the reference's outputs from the call's: on success R21, t21, and vP3D / vbTriangulated sized like mvKeys1 and indexed through mvMatches12[i].first (a keypoint of
// frame 1 is in at most one match, :45-54); on failure everything is left as it was
template <class Tr, class Matches, class Points>
inline bool reconstruct_fill(const ReconstructCall &c, const Matches &vMatches12, size_t nKeys1, typename Tr::Mat33f &R21, typename Tr::Mat31f &t21,
                             Points &vP3D, std::vector<bool> &vbTriangulated) {
    if (!c.result[0]) return false;
    Tr::assign33(R21, c.R21); Tr::assign31(t21, c.t21);
    vP3D.assign(nKeys1, typename Points::value_type()); vbTriangulated.assign(nKeys1, false);
    for (size_t i = 0; i < vMatches12.size(); i++) { const size_t k = (size_t)vMatches12[i].first;
        vP3D[k].x = c.p3d[3*i]; vP3D[k].y = c.p3d[3*i + 1]; vP3D[k].z = c.p3d[3*i + 2];
        vbTriangulated[k] = c.triangulated[i] != 0; }
    return true;
}

// ReconstructH(vbMatchesInliersH, H, mK, R21, t21, vP3D, vbTriangulated, 1.0, 50) (model 0) or ReconstructF(vbMatchesInliersF, F, ...) (model 1) in ONE call.
// Returns what the reference returns; false also on a device or argument error (tsorb_last_error(orbCtx) says what; keep->result[5] is -1 then).
template <class Tr, class Keys, class Matches, class Points>
inline bool reconstruct(void *orbCtx, const Keys &vKeys1, const Keys &vKeys2, const Matches &vMatches12, const std::vector<bool> &vbMatchesInliers, int model,
                        const typename Tr::Mat33f &M21, const typename Tr::Mat33f &K, float sigma, typename Tr::Mat33f &R21, typename Tr::Mat31f &t21,
                        Points &vP3D, std::vector<bool> &vbTriangulated, float minParallax = 1.0f, int minTriangulated = 50, ReconstructCall *keep = 0) {
    ReconstructCall local, &c = keep ? *keep : local;
    reconstruct_gather<Tr>(vKeys1, vKeys2, vMatches12, vbMatchesInliers, M21, K, c);
    const size_t n = (size_t)c.n();
    c.p3d.assign(3*(n ? n : 1), 0.f); c.triangulated.assign(n ? n : 1, 0);
    for (int i = 0; i < 6; i++) c.result[i] = 0;
    const int rc = tsorb_match_two_view_reconstruct(orbCtx, (int)n, c.xy1.data(), c.xy2.data(), c.inlier.data(), model, c.M21, c.K, sigma, minParallax, minTriangulated,
                                                    c.result, c.R21, c.t21, c.p3d.data(), c.triangulated.data(), 0, 0, 0, 0, 0, 0);
    if (rc != TSORB_OK) { c.result[0] = 0; c.result[5] = -1; return false; }
    return reconstruct_fill<Tr>(c, vMatches12, vKeys1.size(), R21, t21, vP3D, vbTriangulated);
}

}  // namespace tsorb_adapter
#endif
