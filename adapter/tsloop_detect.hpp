// tsloop_detect.hpp -- header-only body of loopClosing::DetectLoop (src/loopClosing.cc:119-304) over tsloop_detect_loop (include/tsloop.h): the Levenshtein scan of
// every text the current keyframe observes against every text object of the map, the match lists, the keyframe vote and the candidate walk in ONE call, where the
// reference runs (texts in view) x (texts in the map) string DPs, a sort of all map texts per query and copies of the three co-visibility matrices on the tracking thread.
// C++11, no OpenCV, no Eigen.  KF is the reference's keyframe (mnId, vObvText), the map its map (GetAllMapTexts(), imapkfs), a map text its mapText (mnId, STATE,
// TextMean.mean, vObvkeyframe), MatchRes its MatchmapTextRes {mapObj, dist, score}.  Tr gives
//   static <status> text_bad();                                          // TEXTBAD
//   static double covis(Map *map, int which, int i, int j);              // element (i, j) of co-visibility matrix which = 0, 1, 2 (vM[which](i, j), :232-234) -- an
//                                                                        // element access: no matrix is copied
// (adapter/textslam_detect_traits.hpp over the real types -- a header of its own, because it needs one accessor added to TextSLAM's map.h and nothing else in
// adapter/ does; tests/cxx/mock_loop_detect.hpp over mock ones.)
// What goes to the call is what the reference's loops read and nothing else: the bytes of the strings, the TEXTBAD flags, each query's own object, and per map text the
// ELIGIBLE keyframes among its observers.  Eligibility (:230-245) does not depend on the match, so it is decided once per keyframe instead of once per vote.
// Two stated differences from the reference (include/tsloop.h): a pair of two empty strings is not scored, and equal scores keep the map's order.
#ifndef TSLOOP_DETECT_HPP
#define TSLOOP_DETECT_HPP
#include <stdint.h>
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>
#include "tsloop.h"

namespace tsloop_adapter {

// The flat arrays of one tsloop_detect_loop call and its results
struct PackedDetect {
    std::vector<int32_t> q_off, q_self, m_off, obs_off, obs_kf; std::vector<uint8_t> q_str, m_str, m_skip;
    std::vector<int32_t> q_obs;                                        // per query: its index in curKF->vObvText
    std::vector<int32_t> match_cnt, match_idx, match_dist, kf_score, kf_nobj, cand; std::vector<double> match_score; int32_t n_cand;
    tsloop_detect_problem p;
    int calls;                                                         // 1, or 2 when a list did not fit the first max_match
    PackedDetect() : n_cand(0), calls(0) { p = tsloop_detect_problem(); }
    // sizes the outputs for max_match and points p at everything (every vector keeps a spare element: data() is never NULL)
    void bind(int max_match) {
        const size_t nq = q_self.size(), nk = (size_t)p.n_kf;
        p.max_match = max_match;
        match_cnt.assign(nq + 1, 0); match_idx.assign(nq*(size_t)max_match + 1, 0); match_dist.assign(nq*(size_t)max_match + 1, 0); match_score.assign(nq*(size_t)max_match + 1, 0.0);
        kf_score.assign(nk + 1, 0); kf_nobj.assign(nk + 1, 0); cand.assign((size_t)p.top_n + 1, 0); n_cand = 0;
        q_str.reserve(q_str.size() + 1); m_str.reserve(m_str.size() + 1); m_skip.reserve(m_skip.size() + 1); q_self.reserve(q_self.size() + 1); obs_kf.reserve(obs_kf.size() + 1);
        p.q_off = q_off.data(); p.q_str = q_str.data(); p.q_self = q_self.data(); p.m_off = m_off.data(); p.m_str = m_str.data(); p.m_skip = m_skip.data();
        p.obs_off = obs_off.data(); p.obs_kf = obs_kf.data();
        p.match_cnt = match_cnt.data(); p.match_idx = match_idx.data(); p.match_dist = match_dist.data(); p.match_score = match_score.data();
        p.kf_score = kf_score.data(); p.kf_nobj = kf_nobj.data(); p.n_cand = &n_cand; p.cand = cand.data();
    }
};

// Gathers the call's arguments.  Returns false -- nothing usable in P -- when a string of a query or of a map text exceeds TSLOOP_TEXT_MAX_LEN.
// vObjs receives the ONE copy of GetAllMapTexts() that the call's map indices refer to: the results are mapped back to objects through it, never through a second
// call (on the real map each call is a locked copy, and the map may have changed in between).
template <class Tr, class KF, class Map, class Connects, class Objs>
bool pack_detect_loop(KF *curKF, const std::vector<KF *> &vKFs, Map *map, int MinMatchedWords, const Connects &vConnects, double ScoreThresh_min, bool DoubleCheck_Visible,
                      PackedDetect &P, Objs &vObjs) {
    P = PackedDetect();
    tsloop_default_options_detect(&P.p);                              // thMinStrScore = 0.3 (:122), TopN = 10 (:273)
    P.p.score_thresh_min = ScoreThresh_min; P.p.min_matched_words = MinMatchedWords;
    // eligible keyframes: index in vKFs by mnId (vmnId2vKFs, :130-139), -1 for the current keyframe, a co-visible one or (DoubleCheck_Visible) a connected one
    std::vector<int32_t> elig((size_t)map->imapkfs, -1);
    const int cur = (int)curKF->mnId;
    for (size_t i = 0; i < vKFs.size(); i++) {
        const int id = (int)vKFs[i]->mnId;
        if (id < 0 || (size_t)id >= elig.size()) continue;                                                                             // (the reference indexes vmnId2vKFs unchecked, :137)
        if (id == cur) continue;                                                                                                       // c0
        if (Tr::covis(map, 0, id, cur) != 0 || Tr::covis(map, 1, id, cur) != 0 || Tr::covis(map, 2, id, cur) != 0) continue;           // c2, c3, c4
        if (DoubleCheck_Visible && vConnects.count(vKFs[i])) continue;
        elig[(size_t)id] = (int32_t)i;
    }
    P.p.n_kf = (int32_t)vKFs.size();
    // map texts, in GetAllMapTexts() order
    vObjs = map->GetAllMapTexts();
    P.m_off.assign(1, 0); P.obs_off.assign(1, 0);
    for (size_t m = 0; m < vObjs.size(); m++) {
        const std::string &s = vObjs[m]->TextMean.mean;
        if (s.size() > (size_t)TSLOOP_TEXT_MAX_LEN) return false;
        P.m_str.insert(P.m_str.end(), s.begin(), s.end()); P.m_off.push_back((int32_t)P.m_str.size());
        P.m_skip.push_back(vObjs[m]->STATE == Tr::text_bad() ? 1 : 0);
        const size_t row = P.obs_kf.size();
        for (auto it = vObjs[m]->vObvkeyframe.begin(); it != vObjs[m]->vObvkeyframe.end(); ++it) {
            const size_t id = (size_t)it->first->mnId;
            if (id < elig.size() && elig[id] >= 0) P.obs_kf.push_back(elig[id]);                                                       // c1: out of vKFs
        }
        std::sort(P.obs_kf.begin() + (std::ptrdiff_t)row, P.obs_kf.end());                                                             // (the map is keyed by pointer)
        P.obs_off.push_back((int32_t)P.obs_kf.size());
    }
    P.p.n_map = (int32_t)vObjs.size();
    // queries: the observed texts whose recognition holds no '#' (:159-161)
    P.q_off.assign(1, 0);
    for (size_t i = 0; i < curKF->vObvText.size(); i++) {
        const auto *objCur = curKF->vObvText[i]->obj;
        const std::string &s = objCur->TextMean.mean;
        if (s.find('#') != std::string::npos) continue;
        if (s.size() > (size_t)TSLOOP_TEXT_MAX_LEN) return false;
        int32_t self = -1;
        for (size_t m = 0; m < vObjs.size(); m++) if (vObjs[m]->mnId == objCur->mnId) { self = (int32_t)m; break; }                    // (mnId is unique in the map)
        P.q_str.insert(P.q_str.end(), s.begin(), s.end()); P.q_off.push_back((int32_t)P.q_str.size());
        P.q_self.push_back(self); P.q_obs.push_back((int32_t)i);
    }
    P.p.n_query = (int32_t)P.q_self.size();
    P.bind(P.p.max_match);
    return true;
}

// Runs the call, and once more with the largest match_cnt when a list did not fit.  Returns tsloop_detect_loop's code.
inline int run_detect_loop(void *loopCtx, PackedDetect &P) {
    int rc = tsloop_detect_loop(loopCtx, &P.p); P.calls = 1;
    if (rc == TSLOOP_ERR_ARG && P.p.n_query > 0) {
        const int32_t most = *std::max_element(P.match_cnt.begin(), P.match_cnt.begin() + P.p.n_query);
        if (most > P.p.max_match) { P.bind(most); rc = tsloop_detect_loop(loopCtx, &P.p); P.calls = 2; }
    }
    return rc;
}

// The drop-in body of loopClosing::DetectLoop.  ok = false -- vAllMatchTextRes untouched, an empty vector returned -- leaves the reference's own loop to the caller:
// a recognition string longer than TSLOOP_TEXT_MAX_LEN bytes, or a failed call (tsloop_last_error(loopCtx) says which).
template <class Tr, class KF, class Map, class Connects, class MatchRes>
std::vector<KF *> detect_loop(void *loopCtx, KF *curKF, const std::vector<KF *> &vKFs, Map *map, int MinMatchedWords, const Connects &vConnects, double ScoreThresh_min,
                              bool DoubleCheck_Visible, std::vector<std::vector<MatchRes> > &vAllMatchTextRes, bool &ok, PackedDetect *keep = 0) {
    PackedDetect own; PackedDetect &P = keep ? *keep : own;
    std::vector<KF *> vMatchKFs;
    decltype(map->GetAllMapTexts()) vObjs;
    ok = pack_detect_loop<Tr>(curKF, vKFs, map, MinMatchedWords, vConnects, ScoreThresh_min, DoubleCheck_Visible, P, vObjs);
    if (!ok) return vMatchKFs;
    ok = run_detect_loop(loopCtx, P) == TSLOOP_OK;
    if (!ok) return vMatchKFs;
    vAllMatchTextRes.assign(curKF->vObvText.size(), std::vector<MatchRes>());                      // a skipped observation keeps an empty entry (:145, :161)
    for (size_t q = 0; q < P.q_obs.size(); q++) {
        std::vector<MatchRes> &v = vAllMatchTextRes[(size_t)P.q_obs[q]];
        const size_t at = q*(size_t)P.p.max_match;
        for (int32_t j = 0; j < P.match_cnt[q]; j++) {
            MatchRes r; r.mapObj = vObjs[(size_t)P.match_idx[at + (size_t)j]]; r.dist = (double)P.match_dist[at + (size_t)j]; r.score = P.match_score[at + (size_t)j];
            v.push_back(r);
        }
    }
    for (int32_t j = 0; j < P.n_cand; j++) vMatchKFs.push_back(vKFs[(size_t)P.cand[(size_t)j]]);
    return vMatchKFs;
}

}  // namespace tsloop_adapter
#endif
