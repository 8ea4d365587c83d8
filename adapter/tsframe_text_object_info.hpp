// tsframe_text_object_info.hpp -- header-only replacement of mapText::GetObjectInfo (src/mapText.cc:64-107) for all new text objects of a keyframe:
// tracking::InitialLandmarkerInKF_Text2 (src/tracking.cc:932-957) constructs one mapText per good detection, and each constructor runs
// tool::CalTextinfo on every level, tool::CalNormvec on every level and tool::GetBoxAllPixs on level 0.  Here the good detections are gathered, ONE
// tsframe_text_object_info call runs on the reference keyframe's context (include/tsframe.h), and the result is written into the objects.
// C++11, no OpenCV / Eigen.  Vec2T has a writable operator()(int) (Eigen's Vec2), Mat33T has operator()(int, int) (vK_scale[l]).
// MT is mapText: members vTextDete (vector<vector<Vec2T>>), vTextDeteRay (vector<Vec2T>), statistics (vector<Vec2T>), vRefFeature
// (vector<vector<TF *>>, set by the constructor from vfeatureText), vRefPixs (vector<TF *>), vRefFeatureSTATE (vector<bool>).  TF is TextFeature:
// u, v, level, IdxToRaw, INITIAL, IN, featureInten, featureNInten, feature / ray with a writable operator()(int), neighbour (vector<Vec2T>),
// neighbourRay (vector of ray's type), neighbourInten, neighbourNInten (vector<double>).  The pixel features are allocated with new, as the reference does.
// A level whose ok flag is 0 (fewer than 2 pixels or sigma == 0: the reference's CalNormvec returns false) leaves its features as they were, as the
// reference does; the level-0 pixels then carry featureNInten = 0.0 where the reference divides by zero.
#ifndef TSFRAME_TEXT_OBJECT_INFO_HPP
#define TSFRAME_TEXT_OBJECT_INFO_HPP
#include <stdint.h>
#include <cmath>
#include <cstddef>
#include <type_traits>
#include <vector>
#include "tsframe.h"

namespace tsframe_adapter {

struct ObjectInfoBatch {                                         // the flat arguments and results of one tsframe_text_object_info call
    size_t L;
    std::vector<double> quad, u, v, inten, musigma, ninten, inten8, ninten8, pix_inten, pix_ninten;
    std::vector<int32_t> feat_off, level_off, pix_off, pix_u, pix_v;
    std::vector<uint8_t> ok, in;
    explicit ObjectInfoBatch(size_t n_levels) : L(n_levels), feat_off(1, 0) {}
    size_t size() const { return feat_off.size() - 1; }
    // one object: its four level-0 corners, then its features level by level (add_feature, each level closed by end_level), then end_object
    void begin_object(const double corners[8]) { quad.insert(quad.end(), corners, corners + 8); level_off.push_back(0); }
    void add_feature(double fu, double fv, double fi) { u.push_back(fu); v.push_back(fv); inten.push_back(fi); }
    void end_level() { level_off.push_back((int32_t)(u.size() - (size_t)feat_off.back()*L)); }
    void end_object() {                                          // the slice is the smallest multiple of L that holds the features: pad it
        const size_t m = u.size() - (size_t)feat_off.back()*L, n = (m + L - 1)/L;
        u.resize((size_t)feat_off.back()*L + n*L, 0.0); v.resize(u.size(), 0.0); inten.resize(u.size(), 0.0);
        feat_off.push_back(feat_off.back() + (int32_t)n);
    }
    size_t feature(size_t obj, size_t level, size_t k) const { return (size_t)feat_off[obj]*L + (size_t)level_off[obj*(L + 1) + level] + k; }
    // the capacity of the pixel arrays is the sum of the clamped level-0 boxes, so one call does it
    int run(void *ctx, const std::vector<double> &inv) {
        const size_t n = size();
        int w = 0, h = 0, wl = 0, hl = 0;                        // the context must hold exactly inv.size() == L levels: the layout depends on it
        if (L == 0 || inv.size() != L || tsframe_level_size(ctx, 0, &w, &h) != TSFRAME_OK || tsframe_level_size(ctx, (int)L - 1, &wl, &hl) != TSFRAME_OK ||
            tsframe_level_size(ctx, (int)L, &wl, &hl) == TSFRAME_OK) return TSFRAME_ERR_ARG;
        double cap = 0.0;
        for (size_t i = 0; i < n; i++) {
            double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
            for (int k = 0; k < 4; k++) {
                const double x = quad[8*i + 2*k]*inv[0], y = quad[8*i + 2*k + 1]*inv[0];
                if (!(std::fabs(x) < 1e9) || !(std::fabs(y) < 1e9)) return TSFRAME_ERR_ARG;
                if (x < x0) x0 = x;
                if (x > x1) x1 = x;
                if (y < y0) y0 = y;
                if (y > y1) y1 = y;
            }
            x0 = clamp(std::floor(x0), w); x1 = clamp(std::ceil(x1), w); y0 = clamp(std::floor(y0), h); y1 = clamp(std::ceil(y1), h);
            cap += (x1 - x0 + 1.0)*(y1 - y0 + 1.0);
        }
        if (cap > 2147483647.0) return TSFRAME_ERR_ARG;
        const size_t pc = cap < 1.0 ? 1 : (size_t)cap, nf = u.size();
        musigma.assign(2*n*L, 0.0); ok.assign(n*L, 0); ninten.assign(nf, 0.0); inten8.assign(8*nf, 0.0); ninten8.assign(8*nf, 0.0); in.assign(nf, 0);
        pix_off.assign(n + 1, 0); pix_u.assign(pc, 0); pix_v.assign(pc, 0); pix_inten.assign(pc, 0.0); pix_ninten.assign(pc, 0.0);
        return tsframe_text_object_info(ctx, (int)n, quad.data(), inv.data(), feat_off.data(), level_off.data(), u.data(), v.data(), inten.data(), (int)pc,
                                        musigma.data(), ok.data(), ninten.data(), inten8.data(), ninten8.data(), in.data(),
                                        pix_off.data(), pix_u.data(), pix_v.data(), pix_inten.data(), pix_ninten.data());
    }
private:
    static double clamp(double x, int n) { return x < 0.0 ? 0.0 : (x > (double)(n - 1) ? (double)(n - 1) : x); }
};

// What mapText::GetObjectInfo leaves in object `obj` of the batch: vTextDete[l], vTextDeteRay, statistics[l], the features' INTERVAL8 neighbourhood and
// normalised intensities, vRefPixs, vRefFeatureSTATE.
template <class MT, class Vec2T, class Mat33T>
void fill_object_info(const ObjectInfoBatch &B, size_t obj, const std::vector<Vec2T> &TextDete, const std::vector<double> &inv, const std::vector<Mat33T> &vK, MT *t) {
    static const double DX[8] = { 0, 2, 1, 0, -1, -2, -1, 0 }, DY[8] = { 0, 0, -1, -2, -1, 0, 1, 2 };       // INTERVAL8, tool.cc:1550-1557
    const size_t L = B.L;
    t->vTextDete.assign(L, std::vector<Vec2T>());
    t->statistics.resize(L);
    for (size_t l = 0; l < L; l++) {                             // mapText.cc:73-85
        for (int k = 0; k < 4; k++) { Vec2T p = TextDete[(size_t)k]; p(0) = TextDete[(size_t)k](0)*inv[l]; p(1) = TextDete[(size_t)k](1)*inv[l]; t->vTextDete[l].push_back(p); }
        t->statistics[l](0) = B.musigma[2*(obj*L + l)]; t->statistics[l](1) = B.musigma[2*(obj*L + l) + 1];
    }
    const double fx0 = vK[0](0, 0), fy0 = vK[0](1, 1), cx0 = vK[0](0, 2), cy0 = vK[0](1, 2);
    t->vTextDeteRay.clear();
    for (int k = 0; k < 4; k++) {                                // mapText.cc:87-90
        Vec2T r = TextDete[(size_t)k]; r(0) = (t->vTextDete[0][(size_t)k](0) - cx0)/fx0; r(1) = (t->vTextDete[0][(size_t)k](1) - cy0)/fy0;
        t->vTextDeteRay.push_back(r);
    }
    for (size_t l = 0; l < L && l < t->vRefFeature.size(); l++) {      // tool::CalNormvec -> GetNeighbour, tool.cc:1342-1355, 1540-1567
        if (!B.ok[obj*L + l]) continue;
        const double fx = vK[l](0, 0), fy = vK[l](1, 1), cx = vK[l](0, 2), cy = vK[l](1, 2);
        for (size_t k = 0; k < t->vRefFeature[l].size(); k++) {
            const size_t at = B.feature(obj, l, k);
            auto f = t->vRefFeature[l][k];
            for (int q = 0; q < 8; q++) {
                Vec2T p = TextDete[0]; p(0) = f->u + DX[q]; p(1) = f->v + DY[q];
                f->neighbour.push_back(p);
                auto r = f->ray; r(0) = (p(0) - cx)/fx; r(1) = (p(1) - cy)/fy; r(2) = 1.0;
                f->neighbourRay.push_back(r);
                f->neighbourInten.push_back(B.inten8[8*at + (size_t)q]); f->neighbourNInten.push_back(B.ninten8[8*at + (size_t)q]);
            }
            f->IN = B.in[at] != 0;
            f->featureNInten = B.ninten[at];
            f->INITIAL = true;
        }
    }
    typedef typename std::remove_pointer<typename std::remove_reference<decltype(t->vRefPixs)>::type::value_type>::type TF;
    t->vRefPixs.clear();                                         // tool::GetBoxAllPixs, tool.cc:1305-1335
    for (int32_t k = B.pix_off[obj]; k < B.pix_off[obj + 1]; k++) {
        TF *f = new TF();
        const double pu = (double)B.pix_u[(size_t)k], pv = (double)B.pix_v[(size_t)k];
        f->u = pu; f->v = pv; f->feature(0) = pu; f->feature(1) = pv; f->level = 0; f->IdxToRaw = (int)(k - B.pix_off[obj]); f->INITIAL = false;
        f->ray(0) = (pu - cx0)/fx0; f->ray(1) = (pv - cy0)/fy0; f->ray(2) = 1.0;
        f->IN = true; f->featureInten = B.pix_inten[(size_t)k]; f->featureNInten = B.pix_ninten[(size_t)k];
        t->vRefPixs.push_back(f);
    }
    t->vRefFeatureSTATE = std::vector<bool>(t->vRefFeature.empty() ? 0 : t->vRefFeature[0].size(), true);      // mapText.cc:106
}

// The loop of tracking::InitialLandmarkerInKF_Text2: objs[i0] is the object constructed for detection i0 of the keyframe (its vRefFeature already holds
// vfeatureText[i0]; entries of detections that are not good are not looked at and may be NULL), vTextDete[i0] its four level-0 corners.  ctx: the
// keyframe's context with its image set on vInvScaleFactors.size() levels; vK_scale[l] = the level's K.  Returns TSFRAME_OK or the error of the call (the objects are then untouched).
template <class MT, class Vec2T, class Mat33T>
int text_object_info(void *ctx, const std::vector<bool> &vNGOOD, const std::vector<std::vector<Vec2T> > &vTextDete, const std::vector<MT *> &objs,
                     const std::vector<double> &vInvScaleFactors, const std::vector<Mat33T> &vK_scale) {
    const size_t L = vInvScaleFactors.size();
    if (vTextDete.size() != vNGOOD.size() || objs.size() != vNGOOD.size() || vK_scale.size() != L) return TSFRAME_ERR_ARG;
    ObjectInfoBatch B(L);
    std::vector<size_t> which;
    for (size_t i0 = 0; i0 < vNGOOD.size(); i0++) {
        if (!vNGOOD[i0]) continue;
        if (!objs[i0] || vTextDete[i0].size() != 4 || objs[i0]->vRefFeature.size() != L) return TSFRAME_ERR_ARG;
        double c[8];
        for (int k = 0; k < 4; k++) { c[2*k] = vTextDete[i0][(size_t)k](0); c[2*k + 1] = vTextDete[i0][(size_t)k](1); }
        B.begin_object(c);
        for (size_t l = 0; l < L; l++) {
            for (size_t k = 0; k < objs[i0]->vRefFeature[l].size(); k++)
                B.add_feature(objs[i0]->vRefFeature[l][k]->u, objs[i0]->vRefFeature[l][k]->v, objs[i0]->vRefFeature[l][k]->featureInten);
            B.end_level();
        }
        B.end_object();
        which.push_back(i0);
    }
    if (which.empty()) return TSFRAME_OK;
    const int rc = B.run(ctx, vInvScaleFactors);
    if (rc != TSFRAME_OK) return rc;
    for (size_t j = 0; j < which.size(); j++) fill_object_info(B, j, vTextDete[which[j]], vInvScaleFactors, vK_scale, objs[which[j]]);
    return TSFRAME_OK;
}

}  // namespace tsframe_adapter
#endif
