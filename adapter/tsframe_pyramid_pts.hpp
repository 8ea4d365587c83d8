// tsframe_pyramid_pts.hpp -- header-only replacement of the loop in frame::TextFeaProc (src/frame.cc:359-370): the reference calls
// tool::GetPyramidPts (src/tool.cc:564-710) once per text detection, and the tracking thread calls the scene overload (src/tool.cc:862-980) once
// more for the frame's scene observations (src/tracking.cc:420; also :333-334, :494).  Here the keypoints of all detections -- and, with the second
// overload, the scene observations as a last set -- go to ONE tsframe_pyramid_pts_batch call on the frame's context (include/tsframe.h), and the
// result is split again into the objects the reference leaves behind.  The sets are independent of each other, so the result is the loop's.
// C++11, no OpenCV / Eigen.  KP is any type with float members pt.x, pt.y (cv::KeyPoint); Vec2T has operator()(int) -> double (Eigen's Vec2);
// Mat33T has operator()(int, int) (vK_scale[0]); TF is TextFeature: members u, v, level, IdxToRaw, INITIAL, featureInten, IN, and feature / ray
// with a writable operator()(int); SF is SceneFeature: u, v, feature, level, IdxToRaw.  The features are allocated with new, as the reference does.
#ifndef TSFRAME_PYRAMID_PTS_HPP
#define TSFRAME_PYRAMID_PTS_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "tsframe.h"

namespace tsframe_adapter {

struct PyramidPtsBatch {                                         // the flat arguments and results of one tsframe_pyramid_pts_batch call
    std::vector<int32_t> mode, xy_off, level_off, idx;
    std::vector<float> xy;
    std::vector<double> box, u, v, inten;
    std::vector<uint8_t> in;
    PyramidPtsBatch() : xy_off(1, 0) {}
    void add_set(int m, double x0, double y0, double x1, double y1) {      // then push the set's points with add_point
        mode.push_back(m); xy_off.push_back(xy_off.back());
        box.push_back(x0); box.push_back(y0); box.push_back(x1); box.push_back(y1);
    }
    void add_point(float x, float y) { xy.push_back(x); xy.push_back(y); xy_off.back()++; }
    int run(void *ctx, const std::vector<double> &inv) {
        const size_t L = inv.size(), ns = mode.size(), tot = (size_t)xy_off.back();
        int w = 0, h = 0;                                        // the context must hold exactly inv.size() levels: the output layout depends on it
        if (L == 0 || tsframe_level_size(ctx, (int)L - 1, &w, &h) != TSFRAME_OK || tsframe_level_size(ctx, (int)L, &w, &h) == TSFRAME_OK) return TSFRAME_ERR_ARG;
        level_off.assign(ns*(L + 1), 0); idx.assign(tot*L, 0); u.assign(tot*L, 0.0); v.assign(tot*L, 0.0); inten.assign(tot*L, 0.0); in.assign(tot*L, 0);
        return tsframe_pyramid_pts_batch(ctx, (int)ns, mode.data(), xy_off.data(), xy.data(), box.data(), inv.data(), level_off.data(),
                                         u.data(), v.data(), idx.data(), inten.data(), in.data());
    }
    size_t begin(size_t set, size_t L, size_t level) const { return (size_t)xy_off[set]*L + (size_t)level_off[set*(L + 1) + level]; }
    size_t end(size_t set, size_t L, size_t level) const { return (size_t)xy_off[set]*L + (size_t)level_off[set*(L + 1) + level + 1]; }
};

template <class TF, class KP, class Mat33T>
void fill_text_features(const PyramidPtsBatch &B, size_t set, size_t L, const std::vector<KP> &keys, const Mat33T &K0, std::vector<std::vector<TF *> > &pyr) {
    const double fx = K0(0, 0), fy = K0(1, 1), cx = K0(0, 2), cy = K0(1, 2);
    pyr.assign(L, std::vector<TF *>());
    for (size_t l = 0; l < L; l++) {
        pyr[l].reserve(B.end(set, L, l) - B.begin(set, L, l));
        for (size_t k = B.begin(set, L, l); k < B.end(set, L, l); k++) {
            TF *f = new TF();
            f->u = B.u[k]; f->v = B.v[k]; f->feature(0) = B.u[k]; f->feature(1) = B.v[k];
            f->level = (int)l; f->IdxToRaw = (int)B.idx[k]; f->INITIAL = false;
            const KP &raw = keys[(size_t)B.idx[k]];               // tool.cc:656, copied at the coarser levels (:697)
            f->ray(0) = (raw.pt.x - cx)/fx; f->ray(1) = (raw.pt.y - cy)/fy; f->ray(2) = 1.0;
            f->featureInten = B.inten[k]; f->IN = B.in[k] != 0;
            pyr[l].push_back(f);
        }
    }
}

template <class KP, class Vec2T>
int gather_text_sets(PyramidPtsBatch &B, const std::vector<std::vector<KP> > &vKeysText, const std::vector<Vec2T> &vTextDeteMin, const std::vector<Vec2T> &vTextDeteMax) {
    if (vTextDeteMin.size() != vKeysText.size() || vTextDeteMax.size() != vKeysText.size()) return TSFRAME_ERR_ARG;
    for (size_t i = 0; i < vKeysText.size(); i++) {
        B.add_set(0, vTextDeteMin[i](0), vTextDeteMin[i](1), vTextDeteMax[i](0), vTextDeteMax[i](1));
        for (size_t j = 0; j < vKeysText[i].size(); j++) B.add_point(vKeysText[i][j].pt.x, vKeysText[i][j].pt.y);
    }
    return TSFRAME_OK;
}

// frame::TextFeaProc: out[i][l] = vfeatureText[i][l], the features of detection i at level l.  ctx: the frame's context, with its image set on
// vInvScaleFactors.size() levels; K0 = vK_scale[0].  Returns TSFRAME_OK or the error of the batch call (out is then empty).
template <class TF, class KP, class Vec2T, class Mat33T>
int text_fea_proc(void *ctx, const std::vector<std::vector<KP> > &vKeysText, const std::vector<Vec2T> &vTextDeteMin, const std::vector<Vec2T> &vTextDeteMax,
                  const std::vector<double> &vInvScaleFactors, const Mat33T &K0, std::vector<std::vector<std::vector<TF *> > > &out) {
    out.clear();
    PyramidPtsBatch B;
    int rc = gather_text_sets(B, vKeysText, vTextDeteMin, vTextDeteMax);
    if (rc == TSFRAME_OK) rc = B.run(ctx, vInvScaleFactors);
    if (rc != TSFRAME_OK) return rc;
    out.resize(vKeysText.size());
    for (size_t i = 0; i < vKeysText.size(); i++) fill_text_features(B, i, vInvScaleFactors.size(), vKeysText[i], K0, out[i]);
    return TSFRAME_OK;
}

// The same with the frame's scene observations (SceneObv2d of tracking.cc:420) as a last, mode-1 set: one call per frame serves frame.cc:366 and
// tracking.cc:420.  vSceneObv2d[l] = the SceneFeatures of level l.  The observations travel as float, the ABI's coordinate type (as through tsframe_pyramid_pts).
template <class TF, class SF, class KP, class Vec2T, class Mat33T>
int text_fea_proc(void *ctx, const std::vector<std::vector<KP> > &vKeysText, const std::vector<Vec2T> &vTextDeteMin, const std::vector<Vec2T> &vTextDeteMax,
                  const std::vector<double> &vInvScaleFactors, const Mat33T &K0, std::vector<std::vector<std::vector<TF *> > > &out,
                  const std::vector<Vec2T> &SceneObv2d, std::vector<std::vector<SF *> > &vSceneObv2d) {
    out.clear(); vSceneObv2d.clear();
    PyramidPtsBatch B;
    int rc = gather_text_sets(B, vKeysText, vTextDeteMin, vTextDeteMax);
    if (rc != TSFRAME_OK) return rc;
    B.add_set(1, 0.0, 0.0, 0.0, 0.0);
    for (size_t j = 0; j < SceneObv2d.size(); j++) B.add_point((float)SceneObv2d[j](0), (float)SceneObv2d[j](1));
    rc = B.run(ctx, vInvScaleFactors);
    if (rc != TSFRAME_OK) return rc;
    const size_t L = vInvScaleFactors.size(), s = vKeysText.size();
    out.resize(s);
    for (size_t i = 0; i < s; i++) fill_text_features(B, i, L, vKeysText[i], K0, out[i]);
    vSceneObv2d.assign(L, std::vector<SF *>());
    for (size_t l = 0; l < L; l++)
        for (size_t k = B.begin(s, L, l); k < B.end(s, L, l); k++) {
            SF *f = new SF();
            f->u = B.u[k]; f->v = B.v[k]; f->feature(0) = B.u[k]; f->feature(1) = B.v[k]; f->level = (int)l; f->IdxToRaw = (int)B.idx[k];
            vSceneObv2d[l].push_back(f);
        }
    return TSFRAME_OK;
}

}  // namespace tsframe_adapter
#endif
