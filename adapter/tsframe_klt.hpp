// tsframe_klt.hpp -- header-only replacement of the loop in tracking::TrackNewTextFeat (src/tracking.cc:1752-1785): the reference calls
// cv::calcOpticalFlowPyrLK(TrackedImg, CurImg, Trackedfeat[i0], Curfeat[i0], status, err) once per new text detection, which rebuilds both LK
// pyramids every time.  Here the points of all detections are concatenated, tracked by ONE tsframe_klt_track call between the resident
// pyramids of the two frames' contexts (include/tsframe.h) and split again.  The points are independent of each other, so the result is the
// same as the loop's.  C++11, no OpenCV: Pt is any type with float members x and y (cv::Point2f in TextSLAM, a mock in
// tests/cxx/klt_from_cxx.cpp).  An empty inner vector stays empty, as tracking.cc:1770-1771 leaves it.
#ifndef TSFRAME_KLT_HPP
#define TSFRAME_KLT_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "tsframe.h"

namespace tsframe_adapter {

struct KltOptions {                                              // cv::calcOpticalFlowPyrLK's defaults, which the reference does not change
    int win, max_level, max_iter; double eps, min_eig;
    KltOptions() : win(21), max_level(3), max_iter(30), eps(0.01), min_eig(1e-4) {}
};

// prev_ctx: the context of the frame the points were seen in (cfLastFrame or cfLastKeyframe), cur_ctx: the current frame's.
// cur[i][j] = the tracked position of tracked[i][j]; status (optional) gets OpenCV's status flags in the same shape.
// Returns TSFRAME_OK or the error of tsframe_klt_track (cur is then left with the shape of tracked and the input positions).
template <class Pt>
int track_new_text_feat(void *prev_ctx, void *cur_ctx, const std::vector<std::vector<Pt> > &tracked, std::vector<std::vector<Pt> > &cur,
                        std::vector<std::vector<uint8_t> > *status = 0, const KltOptions &opt = KltOptions()) {
    size_t n = 0;
    for (size_t i = 0; i < tracked.size(); i++) n += tracked[i].size();
    std::vector<float> in(2*n), out(2*n);
    std::vector<uint8_t> st(n, 0);
    size_t at = 0;
    for (size_t i = 0; i < tracked.size(); i++)
        for (size_t j = 0; j < tracked[i].size(); j++, at++) { in[2*at] = tracked[i][j].x; in[2*at + 1] = tracked[i][j].y; }
    out = in;
    const int rc = tsframe_klt_track(prev_ctx, cur_ctx, (int)n, n ? in.data() : 0, opt.win, opt.max_level, opt.max_iter, opt.eps, opt.min_eig,
                                     n ? out.data() : 0, n ? st.data() : 0);
    if (rc != TSFRAME_OK) { out = in; st.assign(n, 0); }
    cur.assign(tracked.size(), std::vector<Pt>());
    if (status) status->assign(tracked.size(), std::vector<uint8_t>());
    at = 0;
    for (size_t i = 0; i < tracked.size(); i++) {
        cur[i].reserve(tracked[i].size());
        for (size_t j = 0; j < tracked[i].size(); j++, at++) {
            Pt q = tracked[i][j];
            q.x = out[2*at]; q.y = out[2*at + 1];
            cur[i].push_back(q);
            if (status) (*status)[i].push_back(st[at]);
        }
    }
    return rc;
}

}  // namespace tsframe_adapter
#endif
