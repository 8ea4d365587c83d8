// tsba_text_labels.hpp -- what optimizer::UpdateTrackedTextBA / UpdateTrackedTextPOSE read of the text label image (optimizer.cc:2251-2257, 2289-2295,
// 2343-2350): its value at the rounded centre of every text detection -- through tsba_text_label_at (include/tsba.h), without the image.
//
//   std::vector<float> vLabel;
//   tsba_adapter::labels_at_centres(ctx, kf, KFCur->vTextDeteCenter, vLabel);        // vLabel[i0] = what img_ptr[0] was for detection i0
//
// Header-only, C++11, no OpenCV.  A centre is anything with  double operator()(int) const  (Eigen's Vec2; tests/cxx's mock Vec2); a list of centres anything
// with size() and operator[] (std::vector with any allocator).  Labels come back as float, as the CV_32F image held them: (int)label and label < 0 in the
// reference's code read the same values.  A centre that rounds to a pixel outside the level-0 image gets -1 (the reference reads out of bounds there).
#ifndef TSBA_TEXT_LABELS_HPP
#define TSBA_TEXT_LABELS_HPP
#include <cmath>
#include <cstdint>
#include <vector>
#include "tsba.h"

namespace tsba_adapter {

// int u = round(Center(0)): C round, half away from zero.  Values that no int holds (and NaN) become -1: outside every image.
inline int32_t centre_px(double c) {
    const double r = std::round(c);
    return (r >= -2147483648.0 && r <= 2147483647.0) ? (int32_t)r : -1;
}

// Several keyframes in ONE call (OptimizeLandmarker's two newest keyframes): labels[s][i] belongs to centre i of centres[s] in keyframe kfs[s].
// Returns the status of tsba_text_label_at; on error labels is left empty.
template <class Centres>
int labels_at_centres(void *ctx, const std::vector<int> &kfs, const std::vector<const Centres *> &centres, std::vector<std::vector<float> > &labels) {
    labels.clear();
    if (kfs.size() != centres.size()) return TSBA_ERR_ARG;
    std::vector<int32_t> kf, px;
    for (size_t s = 0; s < kfs.size(); s++) {
        const Centres &c = *centres[s];
        for (size_t i = 0; i < (size_t)c.size(); i++) { kf.push_back((int32_t)kfs[s]); px.push_back(centre_px(c[i](0))); px.push_back(centre_px(c[i](1))); }
    }
    std::vector<int32_t> lab(kf.size(), -1);
    const int rc = tsba_text_label_at(ctx, /*level*/0, (int)kf.size(), kf.data(), px.data(), lab.data());
    if (rc != TSBA_OK) return rc;
    labels.resize(kfs.size());
    size_t at = 0;
    for (size_t s = 0; s < kfs.size(); s++) {
        const size_t m = (size_t)centres[s]->size();
        labels[s].resize(m);
        for (size_t i = 0; i < m; i++) labels[s][i] = (float)lab[at++];
    }
    return TSBA_OK;
}

// One keyframe: labels[i] belongs to centres[i].
template <class Centres>
int labels_at_centres(void *ctx, int kf, const Centres &centres, std::vector<float> &labels) {
    std::vector<std::vector<float> > out;
    const int rc = labels_at_centres(ctx, std::vector<int>(1, kf), std::vector<const Centres *>(1, &centres), out);
    if (rc != TSBA_OK) { labels.clear(); return rc; }
    labels.swap(out[0]);
    return TSBA_OK;
}

}  // namespace tsba_adapter
#endif
