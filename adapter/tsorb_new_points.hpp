// tsorb_new_points.hpp -- a new keyframe's scene points through ONE tsorb_match_new_points call, and the initializer's window search through ONE
// tsorb_match_search_claim call (include/tsorb.h): the bodies of the two calls at the head of tracking::TrackNewKeyframe (src/tracking.cc:806-812: SearchForTriangular
// :1347-1411, GetForTriangular :1413-1459 with CheckTriangular :1461-1497) and of tracking::SearchForInitializ (:1045-1109).  Header-only, C++11, no OpenCV or Eigen: the
// templates reach the reference's objects through the member names the reference uses, so they compile against the real types inside the TextSLAM tree and against plain
// structs of the same shape (tests/cxx/new_points_from_cxx.cpp).  docs/newpoints_recalled.md states what the calls run.
//
// What each function restates:
//   set_search_grid                 frame::AssignFeaturesToGrid        src/frame.cc:372-394     F2's features as the context's grid (skip it when tsorb_match_set_frame
//                                                                                               has made the resident frame the grid already: grid_is_set)
//   search_for_triangular_and_get   the two calls at tracking.cc:806-812: the queries are the keyframe's features without a map point and outside every text object,
//                                   in index order; vNewptsMatch12, vNewpts, vNewptsMatch and the returned iNewScene are the reference's
//   search_for_initializ            tracking::SearchForInitializ: the queries are F1's octave-0 features; vMatchIdx12 and the returned nMatches are the reference's
// Both return the call's error code (negative) instead of a count when the call fails; the output vectors are then the reference's empty ones (all -1, no points).
//
// Traits (adapter/textslam_traits.hpp has them over the real types):
//   const uint8_t *row(const Descriptors &, int i)     row i of mDescr, 32 bytes
//   Mat31 vec3(double, double, double)
#ifndef TSORB_NEW_POINTS_HPP
#define TSORB_NEW_POINTS_HPP

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

// what one call takes and gives; query k is feature feat[k] of the first frame
struct NewPointsCall {
    std::vector<int32_t> feat, qlev, match12;
    std::vector<float> qxy, qr, p3d;
    std::vector<uint8_t> qdesc, elig2, good;
    double Trw[12], Tcw[12], K[4];
    int32_t n_match, n_good;
    int rc;
    NewPointsCall() : n_match(0), n_good(0), rc(0) { for (int i = 0; i < 12; i++) Trw[i] = Tcw[i] = 0.0; for (int i = 0; i < 4; i++) K[i] = 0.0; }
    int nq() const { return (int)feat.size(); }
    void add(size_t i1, float x, float y, float r, int octave, const uint8_t *d) {
        feat.push_back((int32_t)i1); qxy.push_back(x); qxy.push_back(y); qr.push_back(r); qlev.push_back(octave); qlev.push_back(octave);
        qdesc.insert(qdesc.end(), d, d + 32);
    }
};

template <class T, class Frame>
inline int set_search_grid(void *orbCtx, const Frame &F2) {
    const size_t n = (size_t)F2.iN;
    std::vector<float> kp6(6*n); std::vector<uint8_t> desc(32*n);
    for (size_t i = 0; i < n; i++) {
        kp6[6*i] = F2.vKeys[i].pt.x; kp6[6*i + 1] = F2.vKeys[i].pt.y; kp6[6*i + 2] = F2.vKeys[i].size; kp6[6*i + 3] = F2.vKeys[i].angle; kp6[6*i + 4] = F2.vKeys[i].response;
        kp6[6*i + 5] = (float)F2.vKeys[i].octave;
        const uint8_t *d = T::row(F2.mDescr, (int)i); for (int k = 0; k < 32; k++) desc[32*i + (size_t)k] = d[k];
    }
    return tsorb_match_set_features(orbCtx, n ? kp6.data() : 0, n ? desc.data() : 0, (int)n, F2.mnMinX, F2.mnMaxX, F2.mnMinY, F2.mnMaxY);
}

template <class Pose> inline void pose_rows(const Pose &Tm, double out[12]) { for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) out[4*r + c] = Tm(r, c); }

// vMatchIdx12 = vector<int>(F1.iN, -1) with the queries' matches in their features' places
inline void scatter_matches(const NewPointsCall &c, size_t iN, std::vector<int> &vMatchIdx12) {
    vMatchIdx12.assign(iN, -1);
    for (size_t k = 0; k < c.feat.size() && k < c.match12.size(); k++) vMatchIdx12[(size_t)c.feat[k]] = c.match12[k];
}

// ---- tracking.cc:806-812
template <class T, class KF, class Frame>
inline void gather_triangular_queries(const KF *F1, const Frame &F2, int Win, NewPointsCall &c) {
    c = NewPointsCall();
    const float ScaleORB = 1.2f, radius = Win*ScaleORB;                                                                 // :1364-1365
    for (size_t i1 = 0; i1 < (size_t)F1->iN; i1++) {
        if (F1->vMatches2D3D[i1] >= 0) continue;                                                                       // cond1
        if (F1->vTextObjInfo[i1] >= 0) continue;
        c.add(i1, F1->vKeys[i1].pt.x, F1->vKeys[i1].pt.y, radius, F1->vKeys[i1].octave, T::row(F1->mDescr, (int)i1));
    }
    c.elig2.resize((size_t)F2.iN);
    for (size_t i2 = 0; i2 < (size_t)F2.iN; i2++) c.elig2[i2] = F2.vMatches2D3D[i2] >= 0 ? 0 : 1;                       // cond2
    pose_rows(F1->mTcw, c.Trw); pose_rows(F2.mTcw, c.Tcw);
    c.K[0] = F2.mK(0, 0); c.K[1] = F2.mK(1, 1); c.K[2] = F2.mK(0, 2); c.K[3] = F2.mK(1, 2);
}
// vNewpts / vNewptsMatch: the good rows in query order, which is MatchRaw's order
template <class T, class VP, class VM>
inline void scatter_new_points(const NewPointsCall &c, VP &vNewpts, VM &vNewptsMatch) {
    typedef typename VM::value_type Match;
    for (size_t k = 0; k < c.good.size(); k++) {
        if (!c.good[k]) continue;
        vNewpts.push_back(T::vec3((double)c.p3d[3*k], (double)c.p3d[3*k + 1], (double)c.p3d[3*k + 2]));
        vNewptsMatch.push_back(Match(c.feat[k], c.match12[k]));
    }
}
template <class T, class KF, class Frame, class VP, class VM>
inline int search_for_triangular_and_get(void *orbCtx, const KF *F1, const Frame &F2, int Win, std::vector<int> &vNewptsMatch12, VP &vNewpts, VM &vNewptsMatch,
                                         bool grid_is_set = false, NewPointsCall *keep = 0, int TH_LOW = 50, int thReproj = 9) {
    NewPointsCall c;
    vNewptsMatch12.assign((size_t)F1->iN, -1);
    gather_triangular_queries<T>(F1, F2, Win, c);
    if (!grid_is_set) { c.rc = set_search_grid<T>(orbCtx, F2); if (c.rc != TSORB_OK) { if (keep) *keep = c; return c.rc; } }
    const size_t Q = c.feat.size();
    c.match12.assign(Q, -1); c.p3d.assign(3*Q, 0.f); c.good.assign(Q, 0);
    c.rc = tsorb_match_new_points(orbCtx, (int)Q, Q ? c.qxy.data() : 0, Q ? c.qr.data() : 0, Q ? c.qlev.data() : 0, Q ? c.qdesc.data() : 0, c.elig2.empty() ? 0 : c.elig2.data(),
                                  TH_LOW, 0, 0.0, Q ? c.qxy.data() : 0, c.Trw, c.Tcw, c.K, thReproj, Q ? c.match12.data() : 0, &c.n_match, Q ? c.p3d.data() : 0,
                                  Q ? c.good.data() : 0, &c.n_good);                                                    // ONE call: q_px is qxy, as in the reference
    if (keep) *keep = c;
    if (c.rc != TSORB_OK) return c.rc;
    scatter_matches(c, (size_t)F1->iN, vNewptsMatch12);
    if (c.n_match == 0) return 0;                                                                                      // `if(iNewScene!=0)`
    scatter_new_points<T>(c, vNewpts, vNewptsMatch);
    return c.n_good;
}

// ---- tracking::SearchForInitializ
template <class T, class Frame>
inline void gather_initializ_queries(const Frame &F1, int Win, NewPointsCall &c) {
    c = NewPointsCall();
    for (size_t i1 = 0; i1 < (size_t)F1.iN; i1++) {
        if (F1.vKeys[i1].octave > 0) continue;                                                                         // Cond1
        c.add(i1, F1.vKeys[i1].pt.x, F1.vKeys[i1].pt.y, (float)Win, F1.vKeys[i1].octave, T::row(F1.mDescr, (int)i1));
    }
}
template <class T, class Frame>
inline int search_for_initializ(void *orbCtx, const Frame &F1, const Frame &F2, int Win, std::vector<int> &vMatchIdx12, bool grid_is_set = false, NewPointsCall *keep = 0,
                                int TH_LOW = 50, double ratio = 0.9) {
    NewPointsCall c;
    vMatchIdx12.assign((size_t)F1.iN, -1);
    gather_initializ_queries<T>(F1, Win, c);
    if (!grid_is_set) { c.rc = set_search_grid<T>(orbCtx, F2); if (c.rc != TSORB_OK) { if (keep) *keep = c; return c.rc; } }
    const size_t Q = c.feat.size();
    c.match12.assign(Q, -1);
    c.rc = tsorb_match_search_claim(orbCtx, (int)Q, Q ? c.qxy.data() : 0, Q ? c.qr.data() : 0, Q ? c.qlev.data() : 0, Q ? c.qdesc.data() : 0, 0, TH_LOW, 1, ratio,
                                    Q ? c.match12.data() : 0, 0, &c.n_match);                                           // ONE call
    if (keep) *keep = c;
    if (c.rc != TSORB_OK) return c.rc;
    scatter_matches(c, (size_t)F1.iN, vMatchIdx12);
    return c.n_match;
}

}  // namespace tsorb_adapter
#endif
