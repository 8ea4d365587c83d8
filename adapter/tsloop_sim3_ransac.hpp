// tsloop_sim3_ransac.hpp -- loopClosing::ComputeSim3's step 3 for every loop candidate through one tsloop_sim3_batch call (include/tsloop.h).
// Header-only, C++11, no third-party include; like adapter/tsloop_gather.hpp the templates reach the reference's objects through the member names the
// reference uses (FeatureConvert::posObv / obv2dPred / obv2d.pt, keyframe::mK), so they compile against the real types inside the TextSLAM tree and against
// plain structs of the same shape (tests/cxx/mock_textslam.hpp, tests/cxx/sim3_ransac_from_cxx.cpp).
//
// What each function restates (citations relative to the TextSLAM tree; docs/sim3solver_recalled.md):
//   sim3_num_hypotheses   Sim3Solver::SetRansacParameters(0.99, 20, 300)  src/Sim3Solver.cc:41-57   and iterate(5, ...)'s loop bound, :65-74
//   draw_sim3_triples     the index draws of iterate                      :72-90                    one list of available indices per candidate, not refilled
//   pack_sim3_batch       Sim3Solver's constructor                        :16-38                    posObv, obv2dPred, mK of both keyframes (+ obv2d.pt for the LM)
//   scatter_sim3_batch    loopClosing::ComputeSim3                        src/loopClosing.cc:330-343  OK, gScm, vbInliers, nInliersOpt of one candidate
// What runs in between -- Horn's closed form per hypothesis, CheckInliers, the selection, optimizer::OptimizeSim3 -- is what the library does.
//
// Traits, in addition to those of tsloop_gather.hpp:
//   int random_int(int lo, int hi)      DUtils::Random::RandomInt(lo, hi): uniform in [lo, hi].  Only initializer.cc, tool.cc's index sets and Sim3Solver draw
//                                       from that generator, and nothing between two candidates' Sim3Solvers does: drawing every candidate's triples, candidate
//                                       by candidate in vKFCands order, before the one call leaves every draw what it was.
#ifndef TSLOOP_SIM3_RANSAC_HPP
#define TSLOOP_SIM3_RANSAC_HPP

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "tsloop.h"

namespace tsloop_adapter {

// How many hypotheses iterate(nIterate, ...) runs on N matches after SetRansacParameters(prob, minInliers, maxIts): 0 when N < minInliers (:65-69)
inline int sim3_num_hypotheses(int N, double prob = 0.99, int minInliers = 20, int maxIts = 300, int nIterate = 5) {
    if (N < minInliers) return 0;
    int nIterations;
    if (minInliers == N) nIterations = 1;
    else {
        const float epsilon = (float)minInliers/N;                            // kept in float, :49
        nIterations = (int)std::ceil(std::log(1 - prob)/std::log(1 - std::pow(epsilon, 3)));      // pow(float, int) is computed in double
    }
    int its = nIterations < maxIts ? nIterations : maxIts; if (its < 1) its = 1;           // mRansacMaxIts = max(1, min(nIterations, maxIts)), :55
    return its < nIterate ? its : nIterate;                                   // while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations), :74
}

// H triples of one candidate with N matches, appended to `triple`: randi = RandomInt(0, size - 1), idx = avail[randi], avail[randi] = avail.back(), pop_back
template <class T>
inline void draw_sim3_triples(int N, int H, std::vector<int32_t> &triple) {
    std::vector<int32_t> avail((size_t)N);
    for (int i = 0; i < N; i++) avail[(size_t)i] = i;                         // Tool.InitialVec(N), :72
    for (int h = 0; h < H; h++)
        for (int i = 0; i < 3; i++) {
            const int randi = T::random_int(0, (int)avail.size() - 1);
            triple.push_back(avail[(size_t)randi]);
            avail[(size_t)randi] = avail.back(); avail.pop_back();
        }
}

struct PackedSim3Batch {
    std::vector<int32_t> off, hyp_off, triple, sel, n_inlier_ransac, hyp_count;
    std::vector<double> P1, P2, pred1, pred2, K2, sim_ransac, sim, hyp_sim;
    std::vector<float> uv1, uv2; std::vector<uint8_t> ok, inlier; std::vector<tsloop_report> rep;
    tsloop_sim3_batch_problem p;
    PackedSim3Batch() { std::memset(&p, 0, sizeof(p)); }
};

template <class M33> inline void k4_of(const M33 &mK, double K[4]) { K[0] = mK(0, 0); K[1] = mK(1, 1); K[2] = mK(0, 2); K[3] = mK(1, 2); }

// pKFCur: mpCurrentKF; vKFCands; vvFeatCur[ikf] / vvFeatCan[ikf]: the vFeatCur / vFeatCan SearchMatch gave for candidate ikf (std::vector<FeatureConvert>);
// K = (fx, fy, cx, cy) of optimizer::K (what OptimizeSim3 uses for both sides).  Draws the triples (see random_int above) and sizes the outputs.
template <class T, class KF, class FeatVec>
inline void pack_sim3_batch(const KF *pKFCur, const std::vector<KF *> &vKFCands, const std::vector<FeatVec> &vvFeatCur, const std::vector<FeatVec> &vvFeatCan,
                            const double K[4], bool optimise, PackedSim3Batch &P) {
    const size_t nc = vKFCands.size();
    P.off.assign(1, 0); P.hyp_off.assign(1, 0); P.triple.clear(); P.K2.resize(4*nc);
    P.P1.clear(); P.P2.clear(); P.pred1.clear(); P.pred2.clear(); P.uv1.clear(); P.uv2.clear();
    for (size_t k = 0; k < nc; k++) {
        const FeatVec &f1 = vvFeatCur[k], &f2 = vvFeatCan[k];
        const size_t n = f1.size();                                           // assert(vFeat1.size() == vFeat2.size()), :25
        for (size_t i = 0; i < n; i++) {
            for (int a = 0; a < 3; a++) { P.P1.push_back(f1[i].posObv(a, 0)); P.P2.push_back(f2[i].posObv(a, 0)); }      // mvX3Dc1 / mvX3Dc2, :27-28
            for (int a = 0; a < 2; a++) { P.pred1.push_back(f1[i].obv2dPred(a)); P.pred2.push_back(f2[i].obv2dPred(a)); }   // mvP1im1 / mvP2im2, :29-30
            P.uv1.push_back(f1[i].obv2d.pt.x); P.uv1.push_back(f1[i].obv2d.pt.y); P.uv2.push_back(f2[i].obv2d.pt.x); P.uv2.push_back(f2[i].obv2d.pt.y);
        }
        k4_of(vKFCands[k]->mK, &P.K2[4*k]);                                   // mK2 = pKF2->mK, :23
        const int H = sim3_num_hypotheses((int)n);
        draw_sim3_triples<T>((int)n, H, P.triple);
        P.off.push_back(P.off.back() + (int32_t)n); P.hyp_off.push_back(P.hyp_off.back() + (int32_t)H);
    }
    const size_t n = (size_t)P.off.back(), nh = (size_t)P.hyp_off.back();
    P.ok.assign(nc, 0); P.sel.assign(nc, -1); P.n_inlier_ransac.assign(nc, 0); P.sim_ransac.assign(8*nc, 0.0); P.sim.assign(8*nc, 0.0);
    P.rep.resize(nc); if (nc) std::memset(P.rep.data(), 0, nc*sizeof(tsloop_report));
    P.inlier.assign(n, 0); P.hyp_count.assign(nh, 0); P.hyp_sim.assign(8*nh, 0.0);
    std::memset(&P.p, 0, sizeof(P.p));
    tsloop_default_options_sim3_ransac(&P.p);                                 // SetRansacParameters(., 20, .); MaxError1 = MaxError2 = 45.0
    P.p.n_cand = (int32_t)nc; P.p.optimise = optimise ? 1 : 0;
    P.p.off = P.off.data(); P.p.hyp_off = P.hyp_off.data(); P.p.triple = P.triple.data();
    P.p.P1 = P.P1.data(); P.p.P2 = P.P2.data(); P.p.pred1 = P.pred1.data(); P.p.pred2 = P.pred2.data(); P.p.uv1 = P.uv1.data(); P.p.uv2 = P.uv2.data();
    P.p.K2 = P.K2.data(); k4_of(pKFCur->mK, P.p.K1);                          // mK1 = pKF1->mK, :22
    for (int a = 0; a < 4; a++) P.p.K[a] = K[a];
    P.p.ok = P.ok.data(); P.p.sel = P.sel.data(); P.p.n_inlier_ransac = P.n_inlier_ransac.data(); P.p.sim_ransac = P.sim_ransac.data(); P.p.sim = P.sim.data();
    P.p.rep = P.rep.data(); P.p.inlier = P.inlier.data(); P.p.hyp_count = P.hyp_count.data(); P.p.hyp_sim = P.hyp_sim.data();
}

// after tsloop_sim3_batch, candidate ikf: returns OK (false: vbDiscarded[ikf] = true; continue).  For an OK candidate vbInliers / gScm / nInliersOpt are what
// iterate() and OptimizeSim3 leave (with optimise == 0: what iterate() leaves, nInliersOpt = the RANSAC count).
template <class T, class BoolVec>
inline bool scatter_sim3_batch(const PackedSim3Batch &P, size_t ikf, BoolVec &vbInliers, typename T::Sim3 &gScm, int &nInliersOpt) {
    const size_t a = (size_t)P.off[ikf], b = (size_t)P.off[ikf + 1];
    vbInliers = BoolVec(b - a, false);
    if (!P.ok[ikf]) return false;
    for (size_t i = a; i < b; i++) vbInliers[i - a] = P.inlier[i] != 0;
    const double *s = P.p.optimise ? &P.sim[8*ikf] : &P.sim_ransac[8*ikf];
    gScm = T::sim_make(s, s + 4, s[7]);
    nInliersOpt = P.p.optimise ? P.rep[ikf].n_inlier : P.n_inlier_ransac[ikf];
    return true;
}

}  // namespace tsloop_adapter
#endif
