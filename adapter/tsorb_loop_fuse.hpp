// tsorb_loop_fuse.hpp -- header-only body of loop fusion's window searches over tsorb_match_search_sets (include/tsorb.h): loopClosing::SearchAndFuse_Scene
// (src/loopClosing.cc:1168-1288), which the reference runs once per keyframe of the loop window (SearchAndFuse, :1091-1166), and loopClosing::MatchMore (:1398-1489),
// which it runs once per loop candidate.  Both project map points into a keyframe, call keyframe::GetFeaturesInArea (src/keyframe.cc:217-256) and scan the window with
// DescriptorDistance, on the loop-closing thread; here the searches of ALL keyframes (all candidates) go to one call, and the reference's loops then run on the stored
// results, with every test that depends on what an earlier keyframe's Replace did still made where the reference makes it.
// C++11, no OpenCV, no Eigen.  KF is the reference's keyframe (vKeys, mDescr, mnMinX .. mnMaxY, vMatches2D3D, vTextObjInfo, vTextDeteCorMap, vObvPts, vObvGoodPts,
// AddSceneObserv), the map point its mapPts (FLAG_BAD, ReplaceKF, IsInKeyFrame, GetKFObv, AddObserv, SetReplaceKF, UpdateCovMap_1).  Tr gives
//   static int rows(const Mat &m);  static const uint8_t *row(const Mat &m, int i);               // a descriptor matrix (cv::Mat CV_8U, 32 columns), as tsorb_loop_match.hpp
//   static int fuse_project(KF *kf, const Sim3 &Scw, MapPt *pt, double &u, double &v);            // loopClosing.cc:1172-1181 + :1196-1211, the reference's own expressions
//                                                                                                 // in doubles: FUSE_OK, FUSE_NEG_DEPTH (:1202) or FUSE_OUTSIDE (:1210)
//   static void more_project(KF *KF1, KF *KFMatch2, const Sim3 &gscm, MapPt *pt, double &u, double &v);   // loopClosing.cc:1422-1432
// (adapter/textslam_traits.hpp over the real types; tests/cxx/mock_loop_fuse.hpp over mock ones.)  The projection stays host arithmetic: no decision at an image
// border can differ from the reference's.
#ifndef TSORB_LOOP_FUSE_HPP
#define TSORB_LOOP_FUSE_HPP
#include <stdint.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

enum { FUSE_OK = 0, FUSE_NEG_DEPTH = 1, FUSE_OUTSIDE = 2 };
enum { FUSE_GRID_COLS = 64, FUSE_GRID_ROWS = 48 };                              // FRAME_GRID_COLS x FRAME_GRID_ROWS (include/tsorb.h)

static inline int fuse_hamming(const uint8_t *a, const uint8_t *b) {             // loopClosing::DescriptorDistance: the 256-bit Hamming distance
    int d = 0;
    for (int w = 0; w < 8; w++) { uint32_t x, y; memcpy(&x, a + 4*w, 4); memcpy(&y, b + 4*w, 4); d += __builtin_popcount(x ^ y); }
    return d;
}

// One query's scan on the host: keyframe::GetFeaturesInArea's window and candidate order (window cells column by column, features in index order inside a cell) and the
// strict < of the scan, from the features and the grid bounds alone (a feature's cell is frame::PosInGrid, frame.cc:395-407).  The winner of that order is the smallest
// (distance, cell, index); n features of kp (stride floats apart, x then y), desc 32 bytes a row.
static inline void window_best_host(const float *kp, int stride, const uint8_t *desc, int n, const double bounds[4], float x, float y, float r, const uint8_t *qd,
                                    int &best_idx, int &best_dist, int &cand_cnt) {
    best_idx = -1; best_dist = INT_MAX; cand_cnt = 0;
    const double min_x = bounds[0], min_y = bounds[2], iw = (double)FUSE_GRID_COLS/(bounds[1] - bounds[0]), ih = (double)FUSE_GRID_ROWS/(bounds[3] - bounds[2]);
    const int c0x = std::max(0, (int)std::floor(((double)x - min_x - (double)r)*iw)), c1x = std::min((int)FUSE_GRID_COLS - 1, (int)std::ceil(((double)x - min_x + (double)r)*iw));
    const int c0y = std::max(0, (int)std::floor(((double)y - min_y - (double)r)*ih)), c1y = std::min((int)FUSE_GRID_ROWS - 1, (int)std::ceil(((double)y - min_y + (double)r)*ih));
    if (c0x >= FUSE_GRID_COLS || c1x < 0 || c0y >= FUSE_GRID_ROWS || c1y < 0) return;
    int best_cell = INT_MAX;
    for (int i = 0; i < n; i++) {
        const float fx = kp[(size_t)stride*i], fy = kp[(size_t)stride*i + 1];
        const int px = (int)std::round(((double)fx - min_x)*iw), py = (int)std::round(((double)fy - min_y)*ih);
        if (px < c0x || px > c1x || py < c0y || py > c1y) continue;
        const float dx = fx - x, dy = fy - y;
        if (!(std::fabs(dx) < r && std::fabs(dy) < r)) continue;
        cand_cnt++;
        const int d = fuse_hamming(qd, desc + 32*(size_t)i), cell = px*FUSE_GRID_ROWS + py;
        if (d < best_dist || (d == best_dist && cell < best_cell)) { best_dist = d; best_idx = i; best_cell = cell; }
    }
}

// The arrays of one tsorb_match_search_sets call and its results (qlev = NULL, no candidate lists)
struct WindowSetsCall {
    std::vector<int32_t> foff; std::vector<float> kp6; std::vector<uint8_t> desc; std::vector<double> bounds;       // the sets
    std::vector<uint8_t> qdesc; std::vector<int32_t> qset, qdi; std::vector<float> qxy, qr;                         // the queries
    std::vector<int32_t> best_idx, best_dist, cand_cnt;
    WindowSetsCall() : foff(1, 0) {}
    int n_set() const { return (int)foff.size() - 1; }
    int nq() const { return (int)qset.size(); }
    template <class Tr, class KF> void add_set(const KF *kf) {
        const size_t n = kf->vKeys.size();
        for (size_t i = 0; i < n; i++) { const float k[6] = { kf->vKeys[i].pt.x, kf->vKeys[i].pt.y, 0.f, 0.f, 0.f, 0.f }; kp6.insert(kp6.end(), k, k + 6);
            const uint8_t *p = Tr::row(kf->mDescr, (int)i); desc.insert(desc.end(), p, p + 32); }
        foff.push_back(foff.back() + (int32_t)n);
        const double b[4] = { kf->mnMinX, kf->mnMaxX, kf->mnMinY, kf->mnMaxY }; bounds.insert(bounds.end(), b, b + 4);
    }
    void add_query(int set, int row, float u, float v, float r) { qset.push_back(set); qdi.push_back(row); qxy.push_back(u); qxy.push_back(v); qr.push_back(r); }
    // on_host: every query through window_best_host instead of the device (a machine without one; the same results)
    int run(void *ctx, bool on_host) {
        const size_t n = (size_t)nq();
        best_idx.assign(n, -1); best_dist.assign(n, INT_MAX); cand_cnt.assign(n, 0);
        if (n == 0 || n_set() == 0) return TSORB_OK;
        if (on_host) {
            for (size_t q = 0; q < n; q++) { const int s = qset[q], f0 = foff[(size_t)s];
                window_best_host(kp6.data() + 6*(size_t)f0, 6, desc.data() + 32*(size_t)f0, foff[(size_t)s + 1] - f0, &bounds[4*(size_t)s], qxy[2*q], qxy[2*q + 1], qr[q],
                                 &qdesc[32*(size_t)qdi[q]], best_idx[q], best_dist[q], cand_cnt[q]); }
            return TSORB_OK;
        }
        kp6.reserve(kp6.size() + 1); desc.reserve(desc.size() + 1);                                                  // (never an empty vector's NULL data())
        return tsorb_match_search_sets(ctx, n_set(), foff.data(), kp6.data(), desc.data(), bounds.data(), (int)(qdesc.size()/32), qdesc.data(), (int)n, qset.data(), qdi.data(),
                                       qxy.data(), qr.data(), 0, 0, 0, 0, cand_cnt.data(), best_idx.data(), best_dist.data(), 0);
    }
};

// ------------------------------------------------------------------ SearchAndFuse_Scene
// The descriptor a loop point is searched with (loopClosing.cc:1222-1233): its observation by mpMatchedKF, else by the keyframe vLoopPts maps it to
template <class KF, class MapPt>
bool fuse_desc_source(MapPt *Pt_loop, KF *mpMatchedKF, KF *second, KF *&KF_loopPt, int &Idx_loopKF) {
    if (Pt_loop->GetKFObv(mpMatchedKF, Idx_loopKF)) { KF_loopPt = mpMatchedKF; return true; }
    KF_loopPt = second;
    return Pt_loop->GetKFObv(KF_loopPt, Idx_loopKF);
}
template <class KF> struct FuseQuery {
    int why;                                        // FUSE_OK / FUSE_NEG_DEPTH / FUSE_OUTSIDE: the state-independent tests of :1196-1211
    bool searched;                                  // a window search was made (why == FUSE_OK and a descriptor source existed at gather time)
    float u, v;                                     // what GetFeaturesInArea(const float &, ..) saw
    KF *KF_loopPt; int Idx_loopKF;                  // the descriptor source as it stood at gather time
    int best_idx, best_dist, cand_cnt;
    FuseQuery() : why(FUSE_OK), searched(false), u(0.f), v(0.f), KF_loopPt(0), Idx_loopKF(-1), best_idx(-1), best_dist(INT_MAX), cand_cnt(0) {}
};
template <class KF> struct FuseSceneSearch {
    std::vector<KF *> KFs; std::vector<std::vector<FuseQuery<KF> > > q;       // q[keyframe][loop point in vLoopPts' order]
    WindowSetsCall call; float th;
    int index_of(const KF *kf) const { for (size_t k = 0; k < KFs.size(); k++) if (KFs[k] == kf) return (int)k; return -1; }
};

// Called once before SearchAndFuse's loops.  KFs in the order the reference visits them (mpCurrentKF first when !AddCurrent, then vConnectKFs in map order), Siws their
// corrected Sim3 (mScw, then the map's values); vLoopPts the reference's std::map<mapPts *, keyframe *>.  One set per keyframe, one descriptor row per loop point.
template <class Tr, class KF, class Sims, class LoopPts>
int fuse_scene_search(void *ctx, const std::vector<KF *> &KFs, const Sims &Siws, const LoopPts &vLoopPts, KF *mpMatchedKF, double th, FuseSceneSearch<KF> &out, bool on_host = false) {
    out.KFs = KFs; out.q.assign(KFs.size(), std::vector<FuseQuery<KF> >(vLoopPts.size())); out.call = WindowSetsCall(); out.th = (float)th;
    WindowSetsCall &W = out.call;
    std::vector<KF *> src(vLoopPts.size(), (KF *)0); std::vector<int> src_idx(vLoopPts.size(), -1);
    W.qdesc.assign(32*vLoopPts.size() + 1, 0);
    size_t p = 0;
    for (typename LoopPts::const_iterator it = vLoopPts.begin(); it != vLoopPts.end(); ++it, ++p) {
        KF *k = 0; int idx = -1;
        if (fuse_desc_source(it->first, mpMatchedKF, it->second, k, idx) && idx >= 0) { src[p] = k; src_idx[p] = idx; memcpy(&W.qdesc[32*p], Tr::row(k->mDescr, idx), 32); }
    }
    for (size_t k = 0; k < KFs.size(); k++) {
        W.template add_set<Tr>(KFs[k]);
        p = 0;
        for (typename LoopPts::const_iterator it = vLoopPts.begin(); it != vLoopPts.end(); ++it, ++p) {
            FuseQuery<KF> &Q = out.q[k][p];
            double u = 0, v = 0;
            Q.why = Tr::fuse_project(KFs[k], Siws[k], it->first, u, v);
            if (Q.why != FUSE_OK) continue;
            Q.u = (float)u; Q.v = (float)v; Q.KF_loopPt = src[p]; Q.Idx_loopKF = src_idx[p];
            if (!src[p]) continue;
            Q.searched = true; W.add_query((int)k, (int)p, Q.u, Q.v, out.th);
        }
    }
    const int rc = W.run(ctx, on_host);
    if (rc != TSORB_OK) return rc;
    size_t at = 0;
    for (size_t k = 0; k < KFs.size(); k++) for (p = 0; p < out.q[k].size(); p++) { FuseQuery<KF> &Q = out.q[k][p]; if (!Q.searched) continue;
        Q.best_idx = W.best_idx[at]; Q.best_dist = W.best_dist[at]; Q.cand_cnt = W.cand_cnt[at]; at++; }
    return TSORB_OK;
}

// SearchAndFuse_Scene's body on the stored results: the reference's loop, its tests in its order; only the window scan (:1214-1249) is the stored one.  FLAG_BAD,
// IsInKeyFrame(KF), vMatches2D3D[bestIdx] and ReplaceKF are read HERE, after the earlier keyframes' Replace calls.  A descriptor source that is no longer the recorded
// one (a Replace merged an observation by mpMatchedKF into the loop point) has that one query's scan redone by window_best_host; nRedone counts them.
// mpMap: GetPtFromId(int); vReplacePts: std::map<mapPts *, mapPts *>; M1 as the reference passes it to UpdateCovMap_1.  Returns nFused.
template <class Tr, class KF, class LoopPts, class Map, class ReplacePts, class Mat>
int search_and_fuse_scene(KF *pKF, const FuseSceneSearch<KF> &S, const LoopPts &vLoopPts, KF *mpMatchedKF, KF *mpCurrentKF, Map *mpMap, ReplacePts &vReplacePts, int TH_LOW,
                          Mat &M1, int *nRedone = 0) {
    const int k = S.index_of(pKF);
    if (k < 0 || S.q[(size_t)k].size() != vLoopPts.size()) return -1;
    int nFused = 0, nHasFused = 0, nAdd = 0;
    size_t p = 0;
    for (typename LoopPts::const_iterator iLpt = vLoopPts.begin(); iLpt != vLoopPts.end(); ++iLpt, ++p) {
        typename LoopPts::key_type Pt_loop = iLpt->first;
        if (Pt_loop->FLAG_BAD || Pt_loop->IsInKeyFrame(pKF)) continue;
        const FuseQuery<KF> &Q = S.q[(size_t)k][p];
        if (Q.why != FUSE_OK) continue;                                           // negative depth, projection outside the image
        if (Q.searched && Q.cand_cnt == 0) continue;                              // vIndices.empty(): whatever the descriptor
        int bestIdx = Q.best_idx, bestDist = Q.best_dist, cnt = Q.cand_cnt;
        KF *KF_loopPt = 0; int Idx_loopKF = -1;
        const bool IN = fuse_desc_source(Pt_loop, mpMatchedKF, iLpt->second, KF_loopPt, Idx_loopKF);
        if (!Q.searched || !IN || KF_loopPt != Q.KF_loopPt || Idx_loopKF != Q.Idx_loopKF) {
            if (!IN || Idx_loopKF < 0) continue;                                  // (the reference asserts both)
            const WindowSetsCall &W = S.call; const int f0 = W.foff[(size_t)k];                     // the keyframe's set as it was sent
            window_best_host(W.kp6.data() + 6*(size_t)f0, 6, W.desc.data() + 32*(size_t)f0, W.foff[(size_t)k + 1] - f0, &W.bounds[4*(size_t)k], Q.u, Q.v, S.th,
                             Tr::row(KF_loopPt->mDescr, Idx_loopKF), bestIdx, bestDist, cnt);
            if (nRedone) (*nRedone)++;
        }
        if (cnt == 0) continue;                                                   // vIndices.empty()
        if (bestDist <= TH_LOW) {
            const int PtmnId = pKF->vMatches2D3D[(size_t)bestIdx];
            if (PtmnId < 0) {
                Pt_loop->AddObserv(pKF, bestIdx);
                Pt_loop->SetReplaceKF(mpCurrentKF);
                pKF->AddSceneObserv(Pt_loop, bestIdx);
                Pt_loop->UpdateCovMap_1(pKF, Pt_loop, M1);
                nAdd++;
                continue;
            }
            typename LoopPts::key_type PtRaw = mpMap->GetPtFromId(PtmnId);
            bool ISOLDPT = true;
            if (PtRaw->ReplaceKF) { if (PtRaw->ReplaceKF->mnId == mpCurrentKF->mnId) ISOLDPT = false; }
            if (ISOLDPT) { vReplacePts[Pt_loop] = PtRaw; nFused++; }
            else nHasFused++;
            nHasFused++;
        }
    }
    (void)nHasFused; (void)nAdd;
    return nFused;
}

// ------------------------------------------------------------------ MatchMore
struct MatchMoreResult { std::vector<int> vMatch12; int nMatches; MatchMoreResult() : nMatches(0) {} };         // ready for FeatureConvert_Other, and MatchMore's return value
struct MatchMoreSearch { WindowSetsCall call; std::vector<std::vector<int> > i0; };                              // per candidate: the observations that were searched

// MatchMore for every loop candidate: the projections of all candidates' points into KF1 are gathered with the `continue` conditions of loopClosing.cc:1414-1437 and
// searched in ONE call (one set: KF1; radius 15 * 1.2f), then the claim logic of :1460-1483 runs per candidate.  th_high = 60 is the reference's.
template <class Tr, class KF, class Sims>
int match_more_all(void *ctx, KF *KF1, const std::vector<KF *> &cands, const Sims &gScms, std::vector<MatchMoreResult> &out, bool on_host = false, MatchMoreSearch *keep = 0,
                   double th_high = 60) {
    const float th = 15.0f, radius = th*1.2f;
    MatchMoreSearch own; MatchMoreSearch &M = keep ? *keep : own;
    M.call = WindowSetsCall(); M.i0.assign(cands.size(), std::vector<int>());
    WindowSetsCall &W = M.call;
    W.template add_set<Tr>(KF1);
    for (size_t c = 0; c < cands.size(); c++) {
        KF *KFMatch2 = cands[c];
        for (size_t i0 = 0; i0 < KFMatch2->vObvPts.size(); i0++) {
            if (!KFMatch2->vObvGoodPts[i0]) continue;
            if (KFMatch2->vObvPts[i0]->pt->FLAG_BAD) continue;
            const int idxPt_KF2 = KFMatch2->vObvPts[i0]->idx;
            double u = 0, v = 0;
            Tr::more_project(KF1, KFMatch2, gScms[c], KFMatch2->vObvPts[i0]->pt, u, v);
            if (u < KF1->mnMinX || u > KF1->mnMaxX) continue;
            if (v < KF1->mnMinY || v > KF1->mnMaxY) continue;
            const uint8_t *d = Tr::row(KFMatch2->mDescr, idxPt_KF2);
            W.add_query(0, W.nq(), (float)u, (float)v, radius); W.qdesc.insert(W.qdesc.end(), d, d + 32);
            M.i0[c].push_back((int)i0);
        }
    }
    W.qdesc.reserve(W.qdesc.size() + 1);
    const int rc = W.run(ctx, on_host);
    if (rc != TSORB_OK) return rc;
    out.assign(cands.size(), MatchMoreResult());
    size_t at = 0;
    for (size_t c = 0; c < cands.size(); c++) {
        KF *KFMatch2 = cands[c];
        std::vector<int> vMatch2D3D(KF1->vKeys.size(), -1), vMatch21(KFMatch2->vKeys.size(), -1);
        out[c].vMatch12.assign(KF1->vKeys.size(), -1);
        for (size_t j = 0; j < M.i0[c].size(); j++, at++) {
            const int i0 = M.i0[c][j], idxPt_KF2 = KFMatch2->vObvPts[(size_t)i0]->idx;
            if (W.cand_cnt[at] == 0) continue;                                    // vIndices1.empty()
            const int bestDist = W.best_dist[at], bestIdx1 = W.best_idx[at];
            if (bestDist <= th_high) {
                if (vMatch2D3D[(size_t)bestIdx1] < 0 && vMatch21[(size_t)idxPt_KF2] < 0) {
                    bool f_3D = false;
                    if (KF1->vTextObjInfo[(size_t)bestIdx1] < 0) { if (KF1->vMatches2D3D[(size_t)bestIdx1] >= 0) f_3D = true; }
                    else { if (KF1->vTextDeteCorMap[(size_t)KF1->vTextObjInfo[(size_t)bestIdx1]] >= 0) f_3D = true; }
                    if (f_3D) { out[c].nMatches++; vMatch2D3D[(size_t)bestIdx1] = i0; vMatch21[(size_t)idxPt_KF2] = bestIdx1; out[c].vMatch12[(size_t)bestIdx1] = idxPt_KF2; }
                }
            }
        }
    }
    return TSORB_OK;
}

}  // namespace tsorb_adapter
#endif
