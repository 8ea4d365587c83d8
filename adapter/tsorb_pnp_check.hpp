// tsorb_pnp_check.hpp -- header-only body of tracking::CheckMatch (src/tracking.cc:1499-1579) over tsorb_match_pnp_ransac (include/tsorb.h): the PnP RANSAC that
// TrackWithMotMod / TrackWithOutMod run on the matches of the window search as soon as more than 20 survive (:412-415, :487-490), before GetSceneObv and PoseOptim.
// C++11, no OpenCV, no Eigen.  docs/pnpransac_recalled.md states what cv::solvePnPRansac is taken to do; what runs between the gather and the mask -- the EPnP
// hypotheses, the inlier counts, the loop with its early stop -- is what the library does.
// The templates reach the reference's objects through the member names the reference uses: MapPt = mapPts (RefKF->GetTwc(), GetRaydir(), GetInverD()), Frame = frame
// (vKeys[i].pt.x / .y, mK), matrices through operator()(row, col).  Tr, the traits the other tsorb adapters take, gives
//   static void pnp_subsets(int n, int n_hyp, std::vector<int32_t> &subset);      // the hypotheses' subsets; PnpTraits below restates OpenCV's own draws
// (a caller with another source of subsets overrides it; tests/cxx/pnp_check_from_cxx.cpp uses PnpTraits as it is).
#ifndef TSORB_PNP_CHECK_HPP
#define TSORB_PNP_CHECK_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

// cv::RNG as recalled: state = (uint64)(unsigned)state * 4164903690U + (unsigned)(state >> 32); next() = (unsigned)state; uniform(a, b) = a + next() % (b - a)
struct CvRng {
    uint64_t state;
    explicit CvRng(uint64_t s = (uint64_t)-1) : state(s) {}
    uint32_t next() { state = (uint64_t)(uint32_t)state*4164903690U + (uint32_t)(state >> 32); return (uint32_t)state; }
    int uniform(int a, int b) { return a + (int)(next() % (uint32_t)(b - a)); }
};

// RANSACPointSetRegistrator::getSubset, n_hyp times from one fresh RNG((uint64)-1): 5 draws, a draw equal to an earlier one of the same subset drawn again
// (PnPRansacCallback has no checkSubset), so the subsets are a function of n alone.  n == 5: the one subset 0 .. 4.
inline void pnp_draw_subsets(int n, int n_hyp, std::vector<int32_t> &subset) {
    subset.clear();
    if (n == 5) { for (int i = 0; i < 5; i++) subset.push_back(i); return; }
    CvRng rng;
    for (int h = 0; h < n_hyp; h++) {
        int32_t idx[5];
        for (int i = 0; i < 5; ) {
            const int v = rng.uniform(0, n);
            int j = 0;
            for (; j < i; j++) if (idx[j] == v) break;
            if (j < i) continue;
            idx[i++] = v;
        }
        subset.insert(subset.end(), idx, idx + 5);
    }
}
struct PnpTraits { static void pnp_subsets(int n, int n_hyp, std::vector<int32_t> &subset) { pnp_draw_subsets(n, n_hyp, subset); } };

// What one CheckMatch sends and receives
struct PnpCheckCall {
    std::vector<float> Pw, uv; std::vector<int32_t> subset, hyp_count; std::vector<uint8_t> inlier; double K[4], pose[12]; int32_t result[4];
    int n() const { return (int)(uv.size()/2); }
};

// :1503-1529 and :1554: the matches' world points (pw = Rwr ray / rho + twr in doubles, then the float of OpenCV's CV_32F conversion), their keypoints, and K through
// the float matrix of Tool.EiM332cvMf
template <class MapPt, class Frame>
inline void pnp_gather(const std::vector<MapPt *> &Pts3d, const Frame &F, const std::vector<int> &vMatch3D2D, PnpCheckCall &c) {
    c.Pw.clear(); c.uv.clear();
    for (size_t imatch = 0; imatch < vMatch3D2D.size(); imatch++) {
        if (vMatch3D2D[imatch] < 0) continue;
        const int idx2 = vMatch3D2D[imatch];
        MapPt *pt = Pts3d[imatch];
        const auto Twr = pt->RefKF->GetTwc();
        const auto ray = pt->GetRaydir();
        const double rho = pt->GetInverD();
        for (int r = 0; r < 3; r++) {
            const double pw = ((Twr(r, 0)*ray(0, 0) + Twr(r, 1)*ray(1, 0)) + Twr(r, 2)*ray(2, 0))/rho + Twr(r, 3);
            c.Pw.push_back((float)pw);
        }
        c.uv.push_back((float)F.vKeys[(size_t)idx2].pt.x); c.uv.push_back((float)F.vKeys[(size_t)idx2].pt.y);
    }
    c.K[0] = (double)(float)F.mK(0, 0); c.K[1] = (double)(float)F.mK(1, 1); c.K[2] = (double)(float)F.mK(0, 2); c.K[3] = (double)(float)F.mK(1, 2);
}

// :1561-1576: every match whose mask is 0 is cleared (all of them when the call did not succeed); returns numMatch
inline int pnp_apply_mask(const uint8_t *inlier, bool ok, std::vector<int> &vMatch3D2D) {
    int numMatch = 0, idx = -1;
    for (size_t i = 0; i < vMatch3D2D.size(); i++) {
        if (vMatch3D2D[i] < 0) continue;
        idx++;
        if (ok && inlier[idx]) { numMatch++; continue; }
        vMatch3D2D[i] = -1;
    }
    return numMatch;
}

// The body of tracking::CheckMatch.  called = false: the call cannot be made (fewer than 5 matches, where cv::solvePnPRansac itself gives up, or an argument the
// library refuses) -- vMatch3D2D is untouched, -1 is returned and the reference's own path is the caller's.  A device error also returns -1 with called = true
// and vMatch3D2D untouched (tsorb_last_error(orbCtx) says what).
template <class Tr, class MapPt, class Frame>
inline int check_match(void *orbCtx, const std::vector<MapPt *> &Pts3d, const Frame &F, std::vector<int> &vMatch3D2D, const float &ReproError, bool &called,
                       PnpCheckCall *keep = 0) {
    PnpCheckCall local, &c = keep ? *keep : local;
    pnp_gather(Pts3d, F, vMatch3D2D, c);
    called = false;
    const int n = c.n();
    if (n < 5 || n > TSORB_PNP_MAX_POINTS) return -1;
    const int itCount = 100; const double Con = 0.98;                       // :1549-1550
    Tr::pnp_subsets(n, itCount, c.subset);
    const int n_hyp = (int)(c.subset.size()/5);
    c.inlier.assign((size_t)n, 0); c.hyp_count.assign((size_t)n_hyp, 0);
    const int rc = tsorb_match_pnp_ransac(orbCtx, n, c.Pw.data(), c.uv.data(), c.K, n_hyp, c.subset.data(), (double)ReproError, Con,
                                          c.inlier.data(), c.result, c.pose, c.hyp_count.data(), 0);
    if (rc == TSORB_ERR_ARG) return -1;
    called = true;
    if (rc != TSORB_OK) return -1;
    return pnp_apply_mask(c.inlier.data(), c.result[0] != 0, vMatch3D2D);
}

}  // namespace tsorb_adapter
#endif
