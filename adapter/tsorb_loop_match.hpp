// tsorb_loop_match.hpp -- header-only body of loopClosing::SearchMatch's two matchers (src/loopClosing.cc:738-925) over tsorb_match_brute_text and
// tsorb_match_brute_scene (include/tsorb.h): the reference runs SearchMatch once per loop candidate of ComputeSim3 (:306-377), and inside it one cv::BFMatcher
// per matched text pair and one N1 x N2 scan on the tracking thread; here the text pairs of ALL candidates go to one call and the scans of all candidates to a
// second one.  FeatureConvert_Text / FeatureConvert_Other (pointer chasing) stay in the caller, on what these functions return.
// C++11, no OpenCV, no Eigen.  KF is the reference's keyframe (members vObvText, vKeysText, mDescrText, vTextDete, vKeys, mDescr, vTextObjInfo, vMatches2D3D,
// vTextDeteCorMap, FrameImg.rows / .cols); MatchRes its MatchmapTextRes (member mapObj, with mapObj->GetObvIdx(KF *, std::vector<int> &)).  Tr reads a
// descriptor matrix (cv::Mat CV_8U, 32 columns):
//   static int rows(const Mat &m);                       // m.rows
//   static const uint8_t *row(const Mat &m, int i);      // m.ptr<uint8_t>(i)
// (tests/cxx/loop_match_from_cxx.cpp has them over mock types.)
#ifndef TSORB_LOOP_MATCH_HPP
#define TSORB_LOOP_MATCH_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "tsorb.h"

namespace tsorb_adapter {

struct BruteMatch { int queryIdx, trainIdx; float distance; };                  // the cv::DMatch fields FeatureConvert_Text reads
// One matched text pair of a candidate: observation iObvText of the current keyframe (detection idxCur) against MatchTexts[iMatchRes] seen by the candidate as
// detection idxCan; match12 = FeatureMatch_brute's good_matches, in query order.
struct TextPairMatch { int iObvText, iMatchRes, idxCur, idxCan; std::vector<BruteMatch> match12; };
// A candidate's SearchMatch_Text: its pairs in the reference's loop order and the boxes painted into the two label images (8 doubles a box, one per pair).
struct CandidateTextMatch { std::vector<TextPairMatch> pairs; std::vector<double> quad_cur, quad_can; };

// SearchMatch_Text for every candidate: the pairs are gathered with exactly the `continue` conditions of loopClosing.cc:768-800, matched in ONE call, and split.
template <class Tr, class KF, class MatchRes>
int search_match_text(void *ctx, KF *CurKF, const std::vector<KF *> &vKFCands, const std::vector<std::vector<MatchRes> > &vMatchTexts,
                      std::vector<CandidateTextMatch> &out) {
    out.assign(vKFCands.size(), CandidateTextMatch());
    if (CurKF->vObvText.size() != vMatchTexts.size()) return TSORB_ERR_ARG;     // (the reference asserts it)
    std::vector<int32_t> off1(1, 0), off2(1, 0); std::vector<uint8_t> d1, d2;
    for (size_t ic = 0; ic < vKFCands.size(); ic++) {
        KF *CanKF = vKFCands[ic];
        for (size_t iObvText = 0; iObvText < CurKF->vObvText.size(); iObvText++) {
            const std::vector<int> &vObvIdxCur = CurKF->vObvText[iObvText]->idx;
            if (vObvIdxCur.size() == 0) continue;
            const int idxCur = vObvIdxCur[0];
            const std::vector<MatchRes> &MatchTexts = vMatchTexts[iObvText];
            for (size_t iMatchRes = 0; iMatchRes < MatchTexts.size(); iMatchRes++) {
                std::vector<int> vObvIdxCan;
                const bool FLAG_CANKFOBV = MatchTexts[iMatchRes].mapObj->GetObvIdx(CanKF, vObvIdxCan);
                if (!FLAG_CANKFOBV || vObvIdxCan.size() == 0) continue;
                const int idxCan = vObvIdxCan[0];
                if (CanKF->vKeysText[idxCan].size() <= 1) continue;
                TextPairMatch P; P.iObvText = (int)iObvText; P.iMatchRes = (int)iMatchRes; P.idxCur = idxCur; P.idxCan = idxCan;
                out[ic].pairs.push_back(P);
                const int r1 = Tr::rows(CurKF->mDescrText[idxCur]), r2 = Tr::rows(CanKF->mDescrText[idxCan]);
                for (int r = 0; r < r1; r++) { const uint8_t *p = Tr::row(CurKF->mDescrText[idxCur], r); d1.insert(d1.end(), p, p + 32); }
                for (int r = 0; r < r2; r++) { const uint8_t *p = Tr::row(CanKF->mDescrText[idxCan], r); d2.insert(d2.end(), p, p + 32); }
                off1.push_back(off1.back() + r1); off2.push_back(off2.back() + r2);
                for (int k = 0; k < 4; k++) {                                                       // tool::GetTextLabelMask: the detection's four corners
                    out[ic].quad_cur.push_back(CurKF->vTextDete[idxCur][k](0)); out[ic].quad_cur.push_back(CurKF->vTextDete[idxCur][k](1));
                    out[ic].quad_can.push_back(CanKF->vTextDete[idxCan][k](0)); out[ic].quad_can.push_back(CanKF->vTextDete[idxCan][k](1));
                }
            }
        }
    }
    const int n_pair = (int)off1.size() - 1;
    if (n_pair == 0) return TSORB_OK;
    const size_t nq = (size_t)off1.back();
    std::vector<int32_t> train(nq ? nq : 1), dist(nq ? nq : 1); std::vector<uint8_t> good(nq ? nq : 1);
    d1.resize(d1.size() + 1); d2.resize(d2.size() + 1);                                             // (never an empty vector's NULL data())
    const int rc = tsorb_match_brute_text(ctx, n_pair, off1.data(), d1.data(), off2.data(), d2.data(), train.data(), dist.data(), good.data());
    if (rc != TSORB_OK) return rc;
    size_t p = 0;
    for (size_t ic = 0; ic < out.size(); ic++)
        for (size_t k = 0; k < out[ic].pairs.size(); k++, p++)
            for (int q = off1[p]; q < off1[p + 1]; q++)
                if (good[(size_t)q]) { BruteMatch m; m.queryIdx = q - off1[p]; m.trainIdx = train[(size_t)q]; m.distance = (float)dist[(size_t)q]; out[ic].pairs[k].match12.push_back(m); }
    return TSORB_OK;
}

// Cond1 of SearchMatch_Other (loopClosing.cc:841-850, :867-878): the feature corresponds to 3-D information
template <class KF>
void loop_match_has3d(const KF *kf, std::vector<uint8_t> &has3d) {
    const size_t n = kf->vKeys.size();
    has3d.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (kf->vTextObjInfo[i] < 0) has3d[i] = kf->vMatches2D3D[i] >= 0;
        else has3d[i] = kf->vTextDeteCorMap[(size_t)kf->vTextObjInfo[i]] >= 0;
    }
}
template <class Tr, class KF>
void loop_match_features(const KF *kf, std::vector<float> &xy, std::vector<uint8_t> &desc, std::vector<uint8_t> &has3d) {
    std::vector<uint8_t> h; loop_match_has3d(kf, h);
    for (size_t i = 0; i < kf->vKeys.size(); i++) {
        xy.push_back(kf->vKeys[i].pt.x); xy.push_back(kf->vKeys[i].pt.y);
        const uint8_t *p = Tr::row(kf->mDescr, (int)i); desc.insert(desc.end(), p, p + 32);
    }
    has3d.insert(has3d.end(), h.begin(), h.end());
}

// SearchMatch_Other for every candidate in ONE call, on the boxes search_match_text collected: vMatchIdx12[ic] is the reference's vMatchIdx12 for candidate ic
// (ready for FeatureConvert_Other), nMatches[ic] its nMatches.  TH_LOW = 50 and the 0.9 ratio are the reference's.
template <class Tr, class KF>
int search_match_other(void *ctx, KF *CurKF, const std::vector<KF *> &vKFCands, const std::vector<CandidateTextMatch> &text,
                       std::vector<std::vector<int> > &vMatchIdx12, std::vector<int> &nMatches, int th_low = 50, double ratio = 0.9) {
    const size_t nc = vKFCands.size(), n1 = CurKF->vKeys.size();
    vMatchIdx12.assign(nc, std::vector<int>(n1, -1)); nMatches.assign(nc, 0);
    if (text.size() != nc) return TSORB_ERR_ARG;
    if (nc == 0) return TSORB_OK;
    std::vector<float> xy1, xy2; std::vector<uint8_t> d1, d2, h1, h2; std::vector<int32_t> off2(1, 0), qoff(1, 0); std::vector<double> qcur, qcan;
    loop_match_features<Tr>(CurKF, xy1, d1, h1);
    for (size_t ic = 0; ic < nc; ic++) {
        loop_match_features<Tr>(vKFCands[ic], xy2, d2, h2);
        off2.push_back((int32_t)(xy2.size()/2));
        qcur.insert(qcur.end(), text[ic].quad_cur.begin(), text[ic].quad_cur.end()); qcan.insert(qcan.end(), text[ic].quad_can.begin(), text[ic].quad_can.end());
        if (text[ic].quad_cur.size() != text[ic].quad_can.size()) return TSORB_ERR_ARG;
        qoff.push_back((int32_t)(qcur.size()/8));
    }
    std::vector<int32_t> m12(nc*(n1 ? n1 : 1)), nm(nc);
    xy1.resize(xy1.size() + 1); xy2.resize(xy2.size() + 1); d1.resize(d1.size() + 1); d2.resize(d2.size() + 1); h1.resize(h1.size() + 1); h2.resize(h2.size() + 1);
    qcur.resize(qcur.size() + 1); qcan.resize(qcan.size() + 1);                                     // (never an empty vector's NULL data())
    const int rc = tsorb_match_brute_scene(ctx, vKFCands[0]->FrameImg.cols, vKFCands[0]->FrameImg.rows, (int)n1, xy1.data(), d1.data(), h1.data(), (int)nc, off2.data(),
                                           xy2.data(), d2.data(), h2.data(), qoff.data(), qcur.data(), qcan.data(), th_low, ratio, m12.data(), nm.data());
    if (rc != TSORB_OK) return rc;
    for (size_t ic = 0; ic < nc; ic++) { nMatches[ic] = nm[ic]; for (size_t i = 0; i < n1; i++) vMatchIdx12[ic][i] = m12[ic*n1 + i]; }
    return TSORB_OK;
}

}  // namespace tsorb_adapter
#endif
