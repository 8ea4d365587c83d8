// TEST INFRASTRUCTURE.  What adapter/tsloop_detect.hpp touches of TextSLAM's object graph: a map text's recognition string, state and observers (src/mapText.h:37-58,
// src/setting.h:98-111), a keyframe's observed texts (src/keyframe.h:150), the map's text objects, keyframe count and co-visibility matrices (src/map.h:33-84).
// Types of their own (mock_textslam.hpp's mapText has no TextMean), with the member names of the reference.
#ifndef MOCK_LOOP_DETECT_HPP
#define MOCK_LOOP_DETECT_HPP
#include <cstddef>
#include <map>
#include <string>
#include <vector>

namespace mockdetect {

enum TextStatus { TEXTGOOD = 0, TEXTIMMATURE = 1, TEXTBAD = 2 };
struct TextInfo { std::string mean; double score, score_semantic; int lang; TextInfo() : score(0), score_semantic(0), lang(0) {} };
struct keyframe; struct mapText;
struct TextObservation { mapText *obj; std::vector<int> idx; double cos; };
struct keyframe { long unsigned int mnId; std::vector<TextObservation *> vObvText; keyframe() : mnId(0) {} };
struct mapText {
    TextStatus STATE; long unsigned int mnId; TextInfo TextMean;
    std::map<keyframe *, std::vector<int> > vObvkeyframe;
    mapText() : STATE(TEXTGOOD), mnId(0) {}
};
struct MatchmapTextRes { mapText *mapObj; double dist; double score; };
struct map {
    std::vector<mapText *> vMapTextObjs; int imapkfs;
    std::vector<double> M[3];                                          // M1, M2, M3 (Eigen::MatrixXd, imapkfs x imapkfs), row-major here
    map() : imapkfs(0) {}
    std::vector<mapText *> GetAllMapTexts() { return vMapTextObjs; }
    void resize_kfs(int n) { imapkfs = n; for (int w = 0; w < 3; w++) M[w].assign((size_t)n*(size_t)n, 0.0); }
};

struct Traits {
    static TextStatus text_bad() { return TEXTBAD; }
    static double covis(map *m, int which, int i, int j) { return m->M[which][(size_t)i*(size_t)m->imapkfs + (size_t)j]; }
};

}  // namespace mockdetect
#endif
