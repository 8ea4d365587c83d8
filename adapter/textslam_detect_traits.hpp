// textslam_detect_traits.hpp -- the Traits of adapter/tsloop_detect.hpp over the REAL TextSLAM types.  Lives in the TextSLAM tree, like textslam_traits.hpp, and is kept
// apart from it on purpose: it is the one piece of adapter/ that needs an addition to one of TextSLAM's own headers, and only a translation unit that includes THIS
// header (the body of loopClosing::DetectLoop) depends on that addition -- optimizer_tsba.cc, optimizer_tsloop.cc and the other adapters compile against map.h as it is.
//
// The addition, to src/map.h (public) -- map::M1 .. M3 are private and GetCovMap* return copies of whole matrices:
//     double GetCovMapAt(int which, int i, int j) const { return which == 0 ? M1(i, j) : which == 1 ? M2(i, j) : M3(i, j); }
// Not compiled by this repository: the same templates are compiled and run here against tests/cxx/mock_loop_detect.hpp, whose Traits has exactly these members.
#ifndef TEXTSLAM_DETECT_TRAITS_HPP
#define TEXTSLAM_DETECT_TRAITS_HPP
#include <setting.h>
#include <mapText.h>
#include <map.h>

namespace tsloop_adapter {

struct TextSlamDetectTraits {
    static TextSLAM::TextStatus text_bad() { return TextSLAM::TEXTBAD; }                                               // loopClosing.cc:180
    // element (i, j) of co-visibility matrix which = 0, 1, 2: vM[which](i, j) of loopClosing.cc:232-234, without the copies of GetCovMap_All()
    static double covis(TextSLAM::map *m, int which, int i, int j) { return m->GetCovMapAt(which, i, j); }
};

}  // namespace tsloop_adapter
#endif
