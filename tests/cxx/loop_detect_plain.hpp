// TEST INFRASTRUCTURE.  A mock world for adapter/tsloop_detect.hpp and a plain restatement of the reference's loop on it (std::string texts, the DP table,
// std::stable_sort): what tests/cxx/loop_detect_from_cxx.cpp compares the adapter with, and what tools/diag/detect_loop_time.cpp times the call against.
#ifndef LOOP_DETECT_PLAIN_HPP
#define LOOP_DETECT_PLAIN_HPP
#include <algorithm>
#include <map>
#include <string>
#include <vector>
#include "mock_loop_detect.hpp"

namespace mockdetect {

typedef std::vector<std::vector<MatchmapTextRes> > AllRes;

struct World {
    map M; std::vector<keyframe> kfs; std::vector<mapText> objs; std::vector<TextObservation> obs; keyframe *cur; std::vector<keyframe *> vKFs;
    std::map<keyframe *, int> vConnects; int MinMatchedWords, DoubleCheck; double ScoreThresh_min;
};

// ---- the reference's loop restated on the mock types: strings, the DP table, a stable sort per query, a stable sort of the keyframes, the walk
inline int edit_distance(const std::string &a, const std::string &b) {
    const size_t la = a.size(), lb = b.size();
    int stack[66*66]; std::vector<int> heap;                           // the reference's table is a stack array too, zeroed before it is filled
    int *dp = stack; if ((la + 1)*(lb + 1) > 66*66) { heap.assign((la + 1)*(lb + 1), 0); dp = heap.data(); }
    const size_t w = lb + 1;
    for (size_t i = 0; i <= la; i++) for (size_t j = 0; j <= lb; j++) dp[i*w + j] = 0;
    for (size_t i = 1; i <= la; i++) dp[i*w] = (int)i;
    for (size_t j = 1; j <= lb; j++) dp[j] = (int)j;
    for (size_t i = 1; i <= la; i++) for (size_t j = 1; j <= lb; j++)
        dp[i*w + j] = a[i - 1] == b[j - 1] ? dp[(i - 1)*w + j - 1] : std::min(dp[(i - 1)*w + j - 1], std::min(dp[i*w + j - 1], dp[(i - 1)*w + j])) + 1;
    return dp[la*w + lb];
}
struct Scored { size_t m; double dist, score; };
inline bool by_score(const Scored &a, const Scored &b) { return a.score > b.score; }
struct Voted { size_t k; double score; };
inline bool by_vote(const Voted &a, const Voted &b) { return a.score > b.score; }

inline std::vector<keyframe *> plain_detect(World &W, AllRes &all) {
    const std::vector<mapText *> vObjs = W.M.GetAllMapTexts();
    const int cur = (int)W.cur->mnId;
    std::vector<int> at((size_t)W.M.imapkfs, -1);
    std::vector<Voted> votes; std::vector<std::map<mapText *, int> > seen(W.vKFs.size());
    for (size_t i = 0; i < W.vKFs.size(); i++) { at[(size_t)W.vKFs[i]->mnId] = (int)i; const Voted v = { i, 0.0 }; votes.push_back(v); }
    all.assign(W.cur->vObvText.size(), std::vector<MatchmapTextRes>());
    for (size_t io = 0; io < W.cur->vObvText.size(); io++) {
        mapText *objCur = W.cur->vObvText[io]->obj;
        const std::string text = objCur->TextMean.mean;
        if (text.find("#") < text.length()) continue;
        std::vector<Scored> sc;
        for (size_t m = 0; m < vObjs.size(); m++) {
            Scored s = { m, -1.0, -1.0 };
            const std::string other = vObjs[m]->TextMean.mean;
            const int maxlen = (int)std::max(text.length(), other.length());
            if (vObjs[m]->STATE != TEXTBAD && vObjs[m]->mnId != objCur->mnId && maxlen > 0) {      // (maxlen > 0: the interface's stated difference)
                s.dist = (double)edit_distance(text, other); s.score = ((double)maxlen - s.dist)/(double)maxlen; }
            sc.push_back(s);
        }
        std::stable_sort(sc.begin(), sc.end(), by_score);
        if (sc.empty() || sc[0].score < 0.3) continue;
        const double best = sc[0].score, th = best == 1.0 ? best : std::max(best*2.0/3.0, W.ScoreThresh_min);
        for (size_t r = 0; r < sc.size(); r++) {
            if (sc[r].score < th) break;
            const MatchmapTextRes res = { vObjs[sc[r].m], sc[r].dist, sc[r].score };
            all[io].push_back(res);
            for (std::map<keyframe *, std::vector<int> >::const_iterator it = res.mapObj->vObvkeyframe.begin(); it != res.mapObj->vObvkeyframe.end(); ++it) {
                const int id = (int)it->first->mnId;
                if (id == cur || at[(size_t)id] == -1) continue;
                if (Traits::covis(&W.M, 0, id, cur) != 0 || Traits::covis(&W.M, 1, id, cur) != 0 || Traits::covis(&W.M, 2, id, cur) != 0) continue;
                if (W.DoubleCheck && W.vConnects.count(it->first)) continue;
                votes[(size_t)at[(size_t)id]].score += 1.0; seen[(size_t)at[(size_t)id]][res.mapObj]++;
            }
        }
    }
    std::stable_sort(votes.begin(), votes.end(), by_vote);
    std::vector<keyframe *> out; const int top = std::min(10, (int)votes.size());
    for (size_t r = 0; r < votes.size(); r++) {
        if (votes[r].score <= W.MinMatchedWords) break;
        if ((int)seen[votes[r].k].size() <= W.MinMatchedWords) continue;
        if ((int)out.size() >= top) break;
        if (Traits::covis(&W.M, 0, (int)W.vKFs[votes[r].k]->mnId, cur) > 0) continue;
        out.push_back(W.vKFs[votes[r].k]);
    }
    return out;
}

}  // namespace mockdetect
#endif
