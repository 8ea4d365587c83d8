// TEST INFRASTRUCTURE.  What adapter/tsorb_loop_fuse.hpp touches of TextSLAM's object graph beyond mock_textslam.hpp: a keyframe's features, descriptors, grid bounds and
// 2-D / 3-D tables (src/keyframe.h:86-158), and the observation bookkeeping of a map point that loop fusion changes (src/mapPts.cc:38-47, :78-86, :145-198).
#ifndef MOCK_LOOP_FUSE_HPP
#define MOCK_LOOP_FUSE_HPP
#include <cstddef>
#include <map>
#include <vector>
#include "mock_textslam.hpp"
#include "tsorb_loop_fuse.hpp"

namespace mockfuse {
using mock::Vec3; using mock::Mat31; using mock::Mat33; using mock::Mat44; using mock::KeyPoint; using mock::Sim3_loop;

struct Mat { int rows, cols; std::vector<uint8_t> data; Mat() : rows(0), cols(32) {}                  // cv::Mat CV_8U, 32 columns
             void push_row(const uint8_t *d) { data.insert(data.end(), d, d + 32); rows++; } };
struct CovCount { long adds; CovCount() : adds(0) {} };                                                // stands for the Eigen::MatrixXd M1: the += 1 of UpdateCovMap_1, counted
struct keyframe; struct mapPts;
struct SceneObservation { mapPts *pt; int idx; };

struct keyframe : mock::keyframe {
    std::vector<KeyPoint> vKeys; Mat mDescr;
    double mnMinX, mnMaxX, mnMinY, mnMaxY, fx, fy, cx, cy;
    std::vector<int> vMatches2D3D, vTextObjInfo, vTextDeteCorMap;
    std::vector<SceneObservation *> vObvPts; std::vector<bool> vObvGoodPts;                            // (of this keyframe type: they hide mock::frame's)
    std::vector<std::pair<long, int> > added;                                                          // test record: (point id, feature) of every AddSceneObserv
    keyframe() : mnMinX(0), mnMaxX(640), mnMinY(0), mnMaxY(480), fx(500), fy(500), cx(320), cy(240) {}
    bool IsInImage(const double &x, const double &y) { return x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY; }
    inline void AddSceneObserv(mapPts *scenept, int idx);
    inline void ReplaceMapPt(const size_t &idx, mapPts *mPt);
};
struct mapPts : mock::mapPts {
    bool FLAG_BAD, Flag_Replaced; keyframe *ReplaceKF, *BeReplacedKF; mapPts *ReplacedmPt; std::map<keyframe *, size_t> vObvkeyframe; int iObs;
    mapPts() : FLAG_BAD(false), Flag_Replaced(false), ReplaceKF(0), BeReplacedKF(0), ReplacedmPt(0), iObs(0) {}
    bool GetKFObv(keyframe *KF, int &IdxObserv) { std::map<keyframe *, size_t>::iterator it = vObvkeyframe.find(KF); if (it == vObvkeyframe.end()) return false; IdxObserv = (int)it->second; return true; }
    bool IsInKeyFrame(keyframe *KF) { return vObvkeyframe.count(KF) != 0; }
    void AddObserv(keyframe *KF, int idx) { if (vObvkeyframe.count(KF)) return; vObvkeyframe.insert(std::make_pair(KF, (size_t)idx)); iObs++; }
    void SetReplaceKF(keyframe *KF) { ReplaceKF = KF; }
    void UpdateCovMap_1(keyframe *KF, mapPts *Scenepts, CovCount &M1) {
        for (std::map<keyframe *, size_t>::iterator it = Scenepts->vObvkeyframe.begin(); it != Scenepts->vObvkeyframe.end(); ++it) if (it->first->mnId < KF->mnId) M1.adds++; }
    void Replace(keyframe *KFCur, mapPts *mPt, CovCount &M1) {
        if (mPt->mnId == this->mnId) return;
        std::map<keyframe *, size_t> obs = vObvkeyframe;
        FLAG_BAD = true; Flag_Replaced = true; ReplacedmPt = mPt; BeReplacedKF = KFCur; mPt->SetReplaceKF(KFCur);
        for (std::map<keyframe *, size_t>::iterator it = obs.begin(); it != obs.end(); ++it) UpdateCovMap_1(it->first, mPt, M1);
        for (std::map<keyframe *, size_t>::iterator it = obs.begin(); it != obs.end(); ++it)
            if (!mPt->IsInKeyFrame(it->first)) { it->first->ReplaceMapPt(it->second, mPt); mPt->AddObserv(it->first, (int)it->second); }
    }
};
inline void keyframe::AddSceneObserv(mapPts *scenept, int idx) { SceneObservation *o = new SceneObservation; o->pt = scenept; o->idx = idx; vObvPts.push_back(o); vObvGoodPts.push_back(true);
    added.push_back(std::make_pair((long)scenept->mnId, idx)); }
inline void keyframe::ReplaceMapPt(const size_t &idx, mapPts *mPt) {
    for (size_t i0 = 0; i0 < vObvPts.size(); i0++) { if ((size_t)vObvPts[i0]->idx != idx) continue; vObvPts[i0]->pt = mPt; vObvGoodPts[i0] = true; }
    vMatches2D3D[idx] = (int)mPt->mnId;
}
struct map { std::vector<mapPts *> vMapPoints; mapPts *GetPtFromId(const int &PtmnId) { return vMapPoints[(size_t)PtmnId]; } };

// The Traits adapter/tsorb_loop_fuse.hpp asks for, over these types: the arithmetic of loopClosing.cc:1172-1211 and :1422-1432 on plain arrays
struct Tr {
    static int rows(const Mat &m) { return m.rows; }
    static const uint8_t *row(const Mat &m, int i) { return m.data.data() + 32*(size_t)i; }
    static Vec3 mul(const Mat33 &R, const Vec3 &v) { Vec3 o; for (int i = 0; i < 3; i++) o(i) = R(i, 0)*v(0) + R(i, 1)*v(1) + R(i, 2)*v(2); return o; }
    static int fuse_project(keyframe *KF, const Sim3_loop &Scw, mapPts *Pt_loop, double &u, double &v) {
        Mat33 Rcw; mock::quat_to_R(Scw.r, Rcw);
        Vec3 tcw; for (int i = 0; i < 3; i++) tcw(i) = Scw.t(i)/Scw.s;                                  // [R, t/s]
        const mock::keyframe *Ref = Pt_loop->RefKF;                                                     // Tcr = Tcw * Trw^-1 = Tcw * Twr
        Vec3 Pr; const Vec3 ray = Pt_loop->GetRaydir(); const double rho = Pt_loop->GetInverD();
        for (int i = 0; i < 3; i++) Pr(i) = ray(i)/rho;
        Vec3 Pw = mul(Ref->mRwc, Pr); for (int i = 0; i < 3; i++) Pw(i) += Ref->mtwc(i);
        Vec3 Pc = mul(Rcw, Pw); for (int i = 0; i < 3; i++) Pc(i) += tcw(i);
        if (Pc(2) < 0.0) return tsorb_adapter::FUSE_NEG_DEPTH;
        const double px = KF->fx*Pc(0) + KF->cx*Pc(2), py = KF->fy*Pc(1) + KF->cy*Pc(2);
        u = px/Pc(2); v = py/Pc(2);
        return KF->IsInImage(u, v) ? tsorb_adapter::FUSE_OK : tsorb_adapter::FUSE_OUTSIDE;
    }
    static void more_project(keyframe *KF1, keyframe *KFMatch2, const Sim3_loop &gscm, mapPts *mpt, double &u, double &v) {
        const Vec3 ray = mpt->GetRaydir(); const double invrho = 1.0/mpt->GetInverD();
        Vec3 Pr; for (int i = 0; i < 3; i++) Pr(i) = invrho*ray(i);
        Vec3 Pw = mul(mpt->RefKF->mRwc, Pr); for (int i = 0; i < 3; i++) Pw(i) += mpt->RefKF->mtwc(i);
        Vec3 PKF2 = mul(KFMatch2->mRcw, Pw); for (int i = 0; i < 3; i++) PKF2(i) += KFMatch2->mtcw(i);
        Mat33 Rcm; mock::quat_to_R(gscm.r, Rcm);
        Vec3 P = mul(Rcm, PKF2); for (int i = 0; i < 3; i++) P(i) += gscm.t(i);
        u = (KF1->fx*P(0) + KF1->cx*P(2))/P(2); v = (KF1->fy*P(1) + KF1->cy*P(2))/P(2);
    }
};

}  // namespace mockfuse
#endif
