// TEST INFRASTRUCTURE: loop fusion's window searches through the adapter (adapter/tsorb_loop_fuse.hpp) from C++, over the mock types of mock_loop_fuse.hpp.
//
//   loop_fuse_from_cxx [--host] <out.bin>     builds a mock world twice, runs a plain transcription of loopClosing::SearchAndFuse's scene part (src/loopClosing.cc:1091-1288)
//                                             and of loopClosing::MatchMore (:1398-1489) on one copy and the adapter on the other, and compares vReplacePts, the
//                                             observations added, nFused, vMatch12, nMatches, the FeatureConvert lists and the final state of every point and keyframe.
//                                             --host: the adapter's searches through window_best_host (no device).  out.bin: the arrays of the adapter's two calls and
//                                             their results (dump_io.hpp records; floats as their bits in i32), for the Python mirror.
//                                             exit code 0 and a line "loop fuse from C++: ok <counter>=<n> ..." = equal; the counters are the transcription's branches
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>
#include "mock_loop_fuse.hpp"
#include "dump_io.hpp"

using namespace mockfuse;
static const int TH_LOW = 50;                                                                          // loopClosing.cc:18

// ---- the world
static uint32_t rng_state;
static uint32_t rnd() { rng_state = rng_state*1664525u + 1013904223u; return rng_state >> 8; }
static double urnd(double a, double b) { return a + (b - a)*(double)(rnd() % 100000)/100000.0; }
static void rand_desc(uint8_t *d) { for (int i = 0; i < 32; i++) d[i] = (uint8_t)rnd(); }
static void flip(const uint8_t *src, int nbits, uint8_t *d) { memcpy(d, src, 32); for (int b = 0; b < nbits; b++) { const uint32_t k = rnd() % 256; d[k >> 3] ^= (uint8_t)(1u << (k & 7)); } }

enum { KF_MATCHED = 0, KF_SECOND = 1, KF_CUR = 5, N_KF = 6, N_LOOP = 200, N_FEAT = 300 };
struct World {
    std::vector<keyframe> kfs; std::vector<mapPts> pts; mockfuse::map Map;
    std::map<mapPts *, keyframe *> vLoopPts; std::vector<keyframe *> KFs; std::vector<Sim3_loop> Siws;
    keyframe *mpMatchedKF, *mpCurrentKF; std::vector<keyframe *> cands; std::vector<Sim3_loop> gScms;
    std::vector<std::set<keyframe *> > seen0; std::vector<std::pair<keyframe *, int> > src0;             // per loop point: who observed it, and its descriptor source, at the start
};
static int add_feature(keyframe &K, float x, float y, const uint8_t *d, int m2d3d) {
    KeyPoint kp; kp.pt.x = x; kp.pt.y = y; K.vKeys.push_back(kp); K.mDescr.push_row(d); K.vMatches2D3D.push_back(m2d3d); K.vTextObjInfo.push_back(-1);
    return (int)K.vKeys.size() - 1;
}
static mapPts *new_point(World &W, keyframe *ref) { mapPts p; p.mnId = W.pts.size(); p.RefKF = ref; p.rho = 1.0; p.ray(0) = p.ray(1) = 0; p.ray(2) = 1; W.pts.push_back(p); return &W.pts.back(); }
static void observe(mapPts *p, keyframe *K, int idx) { p->AddObserv(K, idx); SceneObservation *o = new SceneObservation; o->pt = p; o->idx = idx; K->vObvPts.push_back(o); K->vObvGoodPts.push_back(true); }

static void build_world(World &W, uint32_t seed) {
    rng_state = seed;
    W.kfs.resize(N_KF); W.pts.reserve(8192);                                                            // (pointers into both stay valid, and their order is the index order)
    for (int k = 0; k < N_KF; k++) { keyframe &K = W.kfs[(size_t)k]; K.mnId = (unsigned long)k;
        const double a = k == KF_MATCHED ? 0.0 : 0.01*k, pose[7] = { std::cos(a/2), 0, std::sin(a/2), 0, k == KF_MATCHED ? 0.0 : 0.06*k - 0.2, 0.02*k, k == KF_CUR ? 0.05 : 0.0 };
        mock::Traits::set_pose(K, pose); }
    W.mpMatchedKF = &W.kfs[KF_MATCHED]; W.mpCurrentKF = &W.kfs[KF_CUR];
    W.KFs.push_back(W.mpCurrentKF); for (int k = 2; k <= 4; k++) W.KFs.push_back(&W.kfs[(size_t)k]);     // !AddCurrent: the current keyframe first, then vConnectKFs in map order
    for (size_t k = 0; k < W.KFs.size(); k++) { keyframe *K = W.KFs[k]; const double s = 1.05, t[3] = { K->mtcw(0)*s, K->mtcw(1)*s, K->mtcw(2)*s }; double q[4]; mock::Traits::quat_of(K->mRcw, q);
        W.Siws.push_back(mock::Traits::sim_make(q, t, s)); }
    // the loop points and their descriptors
    std::vector<std::vector<uint8_t> > D((size_t)N_LOOP, std::vector<uint8_t>(32));
    for (int p = 0; p < N_LOOP; p++) {
        keyframe *ref = &W.kfs[(size_t)(p & 1)]; mapPts *P = new_point(W, ref);
        const double px = urnd(-60, 700), py = urnd(-40, 520), depth = urnd(2, 6);
        P->ray(0) = (px - 320.0)/500.0; P->ray(1) = (py - 240.0)/500.0; P->ray(2) = 1.0; P->rho = (p % 25 == 7 ? -1.0 : 1.0)/depth; P->FLAG_BAD = p % 40 == 11;
        rand_desc(D[(size_t)p].data());
        keyframe *obs = &W.kfs[(size_t)((p % 4 == 0) ? KF_MATCHED : KF_SECOND)];                      // p % 4 == 0: seen by mpMatchedKF; the others by the second loop keyframe only
        uint8_t d[32]; flip(D[(size_t)p].data(), (int)(rnd() % 9), d);
        const int row = add_feature(*obs, (float)urnd(5, 635), (float)urnd(5, 475), d, (int)P->mnId);
        observe(P, obs, row); if (p % 9 == 4) obs->vObvGoodPts.back() = false;
        W.vLoopPts[P] = obs;
    }
    // the searched keyframes' features: near the projections of the loop points, with the 2-D / 3-D entries that make the loop take its branches
    std::vector<mapPts *> shared((size_t)N_LOOP, (mapPts *)0);
    for (size_t k = 0; k < W.KFs.size(); k++) {
        keyframe *K = W.KFs[k];
        for (int p = 0; p < N_LOOP; p++) {
            mapPts *P = &W.pts[(size_t)p]; double u, v;
            if (Tr::fuse_project(K, W.Siws[k], P, u, v) != tsorb_adapter::FUSE_OK || rnd() % 10 >= 7) continue;
            uint8_t d[32]; flip(D[(size_t)p].data(), (int)(rnd() % 13), d);
            const int i = add_feature(*K, (float)(u + urnd(-2, 2)), (float)(v + urnd(-2, 2)), d, -1);
            const uint32_t kind = rnd() % 8;
            if (kind == 0 || kind == 1) continue;                                                      // no 3-D point yet: an observation is added
            mapPts *X;
            if (kind <= 4) { if (!shared[(size_t)p]) shared[(size_t)p] = new_point(W, K); X = shared[(size_t)p]; }   // one raw point seen by several searched keyframes
            else { X = new_point(W, K);
                if (kind == 5) X->ReplaceKF = W.mpCurrentKF;                                           // already replaced at this loop: ISOLDPT false
                if (kind == 6 && p % 4 != 0) { uint8_t dm[32]; flip(D[(size_t)p].data(), (int)(rnd() % 11), dm);          // also seen by mpMatchedKF: its Replace changes the source
                    observe(X, W.mpMatchedKF, add_feature(*W.mpMatchedKF, (float)urnd(5, 635), (float)urnd(5, 475), dm, (int)X->mnId)); } }
            K->vMatches2D3D[(size_t)i] = (int)X->mnId; observe(X, K, i);
        }
        while ((int)K->vKeys.size() < N_FEAT) { uint8_t d[32]; rand_desc(d); add_feature(*K, (float)urnd(-3, 643), (float)urnd(-3, 483), d, -1); }
    }
    // MatchMore: the current keyframe against the two loop keyframes; some of its features are text features
    keyframe &C = *W.mpCurrentKF; C.vTextDeteCorMap.push_back(2); C.vTextDeteCorMap.push_back(-1); C.vTextDeteCorMap.push_back(0);
    for (size_t i = 0; i < C.vKeys.size(); i++) if (i % 7 == 3) C.vTextObjInfo[i] = (int)(i % 3);
    W.cands.push_back(&W.kfs[KF_MATCHED]); W.cands.push_back(&W.kfs[KF_SECOND]);
    for (size_t c = 0; c < W.cands.size(); c++) { keyframe *K = W.cands[c]; Sim3_loop a = mock::Traits::sim_of_pose(C.mRcw, C.mtcw, 1.0), b = mock::Traits::sim_of_pose(K->mRcw, K->mtcw, 1.0);
        W.gScms.push_back(a*b.inverse()); }
    for (size_t i = 0; i < W.pts.size(); i++) W.Map.vMapPoints.push_back(&W.pts[i]);
    for (int p = 0; p < N_LOOP; p++) { mapPts *P = &W.pts[(size_t)p]; std::set<keyframe *> s; for (std::map<keyframe *, size_t>::iterator it = P->vObvkeyframe.begin(); it != P->vObvkeyframe.end(); ++it) s.insert(it->first);
        W.seen0.push_back(s); keyframe *k = 0; int idx = -1; tsorb_adapter::fuse_desc_source(P, W.mpMatchedKF, W.vLoopPts[P], k, idx); W.src0.push_back(std::make_pair(k, idx)); }
}

// ---- the reference's loops, transcribed over the mock types
struct Grid { std::vector<size_t> cell[64][48]; double iw, ih; };
static void assign_features_to_grid(const keyframe *K, Grid &G) {                                      // frame::AssignFeaturesToGrid / PosInGrid (frame.cc:372-407)
    G.iw = 64.0/(K->mnMaxX - K->mnMinX); G.ih = 48.0/(K->mnMaxY - K->mnMinY);
    for (size_t i = 0; i < K->vKeys.size(); i++) { const int px = (int)std::round((K->vKeys[i].pt.x - K->mnMinX)*G.iw), py = (int)std::round((K->vKeys[i].pt.y - K->mnMinY)*G.ih);
        if (px >= 0 && px < 64 && py >= 0 && py < 48) G.cell[px][py].push_back(i); }
}
static std::vector<size_t> get_features_in_area(const keyframe *K, const Grid &G, const float &x, const float &y, const float &r) {      // keyframe.cc:217-256
    std::vector<size_t> vIndices;
    const int nMinCellX = std::max(0, (int)std::floor((x - K->mnMinX - r)*G.iw)); if (nMinCellX >= 64) return vIndices;
    const int nMaxCellX = std::min(63, (int)std::ceil((x - K->mnMinX + r)*G.iw)); if (nMaxCellX < 0) return vIndices;
    const int nMinCellY = std::max(0, (int)std::floor((y - K->mnMinY - r)*G.ih)); if (nMinCellY >= 48) return vIndices;
    const int nMaxCellY = std::min(47, (int)std::ceil((y - K->mnMinY + r)*G.ih)); if (nMaxCellY < 0) return vIndices;
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) for (int iy = nMinCellY; iy <= nMaxCellY; iy++) { const std::vector<size_t> &vCell = G.cell[ix][iy];
        for (size_t j = 0; j < vCell.size(); j++) { const KeyPoint &kp = K->vKeys[vCell[j]]; const float distx = kp.pt.x - x, disty = kp.pt.y - y;
            if (std::fabs(distx) < r && std::fabs(disty) < r) vIndices.push_back(vCell[j]); } }
    return vIndices;
}
struct Counters { long skipped, source_changed, added, not_old, neg_depth, outside, empty; Counters() : skipped(0), source_changed(0), added(0), not_old(0), neg_depth(0), outside(0), empty(0) {} };

static int ref_search_and_fuse_scene(World &W, keyframe *KF, const Sim3_loop &Scw, std::map<mapPts *, mapPts *> &vReplacePts, double th, CovCount &M1, Counters &C) {
    Grid *G = new Grid; assign_features_to_grid(KF, *G);
    int nFused = 0, nHasFused = 0, nAdd = 0, p = 0;
    for (std::map<mapPts *, keyframe *>::const_iterator iLpt = W.vLoopPts.begin(); iLpt != W.vLoopPts.end(); ++iLpt, ++p) {
        mapPts *Pt_loop = iLpt->first;
        if (Pt_loop->FLAG_BAD || Pt_loop->IsInKeyFrame(KF)) { if (!Pt_loop->FLAG_BAD && !W.seen0[(size_t)p].count(KF)) C.skipped++; continue; }
        double u, v;
        const int why = Tr::fuse_project(KF, Scw, Pt_loop, u, v);
        if (why == tsorb_adapter::FUSE_NEG_DEPTH) { C.neg_depth++; continue; }
        if (why == tsorb_adapter::FUSE_OUTSIDE) { C.outside++; continue; }
        double radius = th;
        const std::vector<size_t> vIndices = get_features_in_area(KF, *G, (float)u, (float)v, (float)radius);
        if (vIndices.empty()) { C.empty++; continue; }
        int Idx_loopKF; keyframe *KF_loopPt;
        if (Pt_loop->GetKFObv(W.mpMatchedKF, Idx_loopKF)) KF_loopPt = W.mpMatchedKF;
        else { KF_loopPt = iLpt->second; if (!Pt_loop->GetKFObv(KF_loopPt, Idx_loopKF)) { fprintf(stderr, "a loop point without a descriptor source\n"); exit(3); } }
        if (KF_loopPt != W.src0[(size_t)p].first || Idx_loopKF != W.src0[(size_t)p].second) C.source_changed++;
        const uint8_t *dMP = Tr::row(KF_loopPt->mDescr, Idx_loopKF);
        int bestDist = INT_MAX, bestIdx = -1;
        for (std::vector<size_t>::const_iterator vit = vIndices.begin(); vit != vIndices.end(); ++vit) { const int dist = tsorb_adapter::fuse_hamming(dMP, Tr::row(KF->mDescr, (int)*vit));
            if (dist < bestDist) { bestDist = dist; bestIdx = (int)*vit; } }
        if (bestDist <= TH_LOW) {
            const int PtmnId = KF->vMatches2D3D[(size_t)bestIdx];
            if (PtmnId < 0) { Pt_loop->AddObserv(KF, bestIdx); Pt_loop->SetReplaceKF(W.mpCurrentKF); KF->AddSceneObserv(Pt_loop, bestIdx); Pt_loop->UpdateCovMap_1(KF, Pt_loop, M1); nAdd++; C.added++; continue; }
            mapPts *PtRaw = W.Map.GetPtFromId(PtmnId);
            bool ISOLDPT = true;
            if (PtRaw->ReplaceKF) { if (PtRaw->ReplaceKF->mnId == W.mpCurrentKF->mnId) ISOLDPT = false; }
            if (ISOLDPT) { vReplacePts[Pt_loop] = PtRaw; nFused++; } else { nHasFused++; C.not_old++; }
            nHasFused++;
        }
    }
    delete G; (void)nHasFused; (void)nAdd;
    return nFused;
}
static int ref_match_more(keyframe *KF1, keyframe *KFMatch2, const Sim3_loop &gscm, std::vector<int> &vMatch12) {
    const float th = 15.0f; const double th_high = 60;
    Grid *G = new Grid; assign_features_to_grid(KF1, *G);
    const std::vector<SceneObservation *> vPts = KFMatch2->vObvPts;
    std::vector<int> vMatch2D3D(KF1->vKeys.size(), -1), vMatch3D2D(vPts.size(), -1), vMatch21(KFMatch2->vKeys.size(), -1);
    vMatch12.assign(KF1->vKeys.size(), -1);
    int nMatches = 0;
    for (size_t i0 = 0; i0 < vPts.size(); i0++) {
        if (!KFMatch2->vObvGoodPts[i0]) continue;
        if (vPts[i0]->pt->FLAG_BAD) continue;
        const int idxPt_KF2 = KFMatch2->vObvPts[i0]->idx;
        double u, v; Tr::more_project(KF1, KFMatch2, gscm, vPts[i0]->pt, u, v);
        if (u < KF1->mnMinX || u > KF1->mnMaxX) continue;
        if (v < KF1->mnMinY || v > KF1->mnMaxY) continue;
        const float radius = th*1.2f;
        const std::vector<size_t> vIndices1 = get_features_in_area(KF1, *G, (float)u, (float)v, radius);
        if (vIndices1.empty()) continue;
        const uint8_t *dMP = Tr::row(KFMatch2->mDescr, idxPt_KF2);
        int bestDist = INT_MAX, bestIdx1 = -1;
        for (size_t j = 0; j < vIndices1.size(); j++) { const int dist = tsorb_adapter::fuse_hamming(dMP, Tr::row(KF1->mDescr, (int)vIndices1[j])); if (dist < bestDist) { bestDist = dist; bestIdx1 = (int)vIndices1[j]; } }
        if (bestDist <= th_high) {
            if (vMatch2D3D[(size_t)bestIdx1] < 0 && vMatch21[(size_t)idxPt_KF2] < 0) {
                bool f_3D = false;
                if (KF1->vTextObjInfo[(size_t)bestIdx1] < 0) { if (KF1->vMatches2D3D[(size_t)bestIdx1] >= 0) f_3D = true; }
                else { const int idxDete = KF1->vTextObjInfo[(size_t)bestIdx1]; if (KF1->vTextDeteCorMap[(size_t)idxDete] >= 0) f_3D = true; }
                if (f_3D) { nMatches++; vMatch3D2D[i0] = bestIdx1; vMatch2D3D[(size_t)bestIdx1] = (int)i0; vMatch21[(size_t)idxPt_KF2] = bestIdx1; vMatch12[(size_t)bestIdx1] = idxPt_KF2; }
            }
        }
    }
    delete G;
    return nMatches;
}
// FeatureConvert_Other (loopClosing.cc:976-1004) on the mock world: a feature's FlagTS and the id of its point / text object; the pairs it keeps
static void feature_convert_other(const std::vector<int> &vMatchIdx12, keyframe *KF1, keyframe *KF2, std::vector<long> &out) {
    for (size_t ifeat = 0; ifeat < vMatchIdx12.size(); ifeat++) { if (vMatchIdx12[ifeat] < 0) continue;
        const int idx1 = (int)ifeat, idx2 = vMatchIdx12[ifeat];
        const int ts1 = KF1->vTextObjInfo[(size_t)idx1] >= 0, ts2 = KF2->vTextObjInfo[(size_t)idx2] >= 0;
        const long id1 = ts1 ? KF1->vTextDeteCorMap[(size_t)KF1->vTextObjInfo[(size_t)idx1]] : KF1->vMatches2D3D[(size_t)idx1], id2 = ts2 ? KF2->vTextDeteCorMap[(size_t)KF2->vTextObjInfo[(size_t)idx2]] : KF2->vMatches2D3D[(size_t)idx2];
        if (ts1 == ts2 && id1 == id2) continue;
        const long rec[6] = { idx1, idx2, ts1, ts2, id1, id2 }; out.insert(out.end(), rec, rec + 6); }
}

// everything a run leaves behind, as numbers (ids, never pointers)
static void signature(World &W, std::vector<long> &s) {
    for (size_t i = 0; i < W.pts.size(); i++) { mapPts &P = W.pts[i]; s.push_back(P.FLAG_BAD); s.push_back(P.ReplaceKF ? (long)P.ReplaceKF->mnId : -1); s.push_back(P.ReplacedmPt ? (long)P.ReplacedmPt->mnId : -1); s.push_back(P.iObs);
        std::vector<std::pair<long, long> > o; for (std::map<keyframe *, size_t>::iterator it = P.vObvkeyframe.begin(); it != P.vObvkeyframe.end(); ++it) o.push_back(std::make_pair((long)it->first->mnId, (long)it->second));
        std::sort(o.begin(), o.end()); for (size_t k = 0; k < o.size(); k++) { s.push_back(o[k].first); s.push_back(o[k].second); } s.push_back(-99); }
    for (size_t k = 0; k < W.kfs.size(); k++) { keyframe &K = W.kfs[k]; for (size_t i = 0; i < K.vMatches2D3D.size(); i++) s.push_back(K.vMatches2D3D[i]);
        for (size_t i = 0; i < K.vObvPts.size(); i++) { s.push_back((long)K.vObvPts[i]->pt->mnId); s.push_back(K.vObvPts[i]->idx); s.push_back(K.vObvGoodPts[i]); }
        for (size_t i = 0; i < K.added.size(); i++) { s.push_back(K.added[i].first); s.push_back(K.added[i].second); } s.push_back(-98); }
}
static void put_f32(FILE *f, const char *name, const std::vector<float> &v) { put(f, name, 1, v.data(), v.size()); }
static void dump_call(FILE *f, const char *pre, const tsorb_adapter::WindowSetsCall &W) {
    std::string p(pre);
    put(f, (p + "foff").c_str(), 1, W.foff.data(), W.foff.size()); put_f32(f, (p + "kp6").c_str(), W.kp6); put(f, (p + "desc").c_str(), 2, W.desc.data(), W.desc.size());
    put(f, (p + "bounds").c_str(), 0, W.bounds.data(), W.bounds.size()); put(f, (p + "qdesc").c_str(), 2, W.qdesc.data(), 32*(W.qdesc.size()/32));
    put(f, (p + "qset").c_str(), 1, W.qset.data(), W.qset.size()); put(f, (p + "qdi").c_str(), 1, W.qdi.data(), W.qdi.size()); put_f32(f, (p + "qxy").c_str(), W.qxy); put_f32(f, (p + "qr").c_str(), W.qr);
    put(f, (p + "best_idx").c_str(), 1, W.best_idx.data(), W.best_idx.size()); put(f, (p + "best_dist").c_str(), 1, W.best_dist.data(), W.best_dist.size());
    put(f, (p + "cand_cnt").c_str(), 1, W.cand_cnt.data(), W.cand_cnt.size());
}

int main(int argc, char **argv) {
    bool on_host = false; const char *outp = 0;
    for (int a = 1; a < argc; a++) { if (strcmp(argv[a], "--host") == 0) on_host = true; else outp = argv[a]; }
    if (!outp) { fprintf(stderr, "usage: %s [--host] out.bin\n", argv[0]); return 2; }
    World *A = new World, *B = new World; build_world(*A, 4711u); build_world(*B, 4711u);
    { std::vector<long> a, b; signature(*A, a); signature(*B, b); if (a != b || a.size() < 1000) { fprintf(stderr, "the two worlds differ\n"); return 1; } }
    void *ctx = 0;
    if (!on_host) { const int rc = tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0); if (rc != TSORB_OK) { fprintf(stderr, "tsorb_create: %d\n", rc); return 1; } }
    const char *err = "";
#define FAIL(msg) do { fprintf(stderr, "%s (%s)\n", msg, (ctx && tsorb_last_error(ctx)) ? tsorb_last_error(ctx) : err); return 1; } while (0)

    // MatchMore (it changes nothing, so it goes first)
    std::vector<tsorb_adapter::MatchMoreResult> mm; tsorb_adapter::MatchMoreSearch mms;
    if (tsorb_adapter::match_more_all<Tr>(ctx, B->mpCurrentKF, B->cands, B->gScms, mm, on_host, &mms) != TSORB_OK) FAIL("match_more_all failed");
    long mm_matches = 0, mm_text = 0, mm_convert = 0;
    for (size_t c = 0; c < A->cands.size(); c++) {
        std::vector<int> vMatch12; const int nMatches = ref_match_more(A->mpCurrentKF, A->cands[c], A->gScms[c], vMatch12);
        if (vMatch12 != mm[c].vMatch12 || nMatches != mm[c].nMatches) FAIL("MatchMore: vMatch12 / nMatches differ");
        std::vector<long> fa, fb; feature_convert_other(vMatch12, A->mpCurrentKF, A->cands[c], fa); feature_convert_other(mm[c].vMatch12, B->mpCurrentKF, B->cands[c], fb);
        if (fa != fb) FAIL("MatchMore: the FeatureConvert lists differ");
        mm_matches += nMatches; mm_convert += (long)fa.size()/6; for (size_t i = 0; i < fa.size(); i += 6) mm_text += fa[i + 2];
    }

    // SearchAndFuse, the scene part: the transcription on A ...
    Counters C; CovCount M1a, M1b; std::vector<std::vector<std::pair<long, long> > > repA, repB; std::vector<int> nFusedA, nFusedB;
    for (size_t k = 0; k < A->KFs.size(); k++) {
        std::map<mapPts *, mapPts *> vReplacePts;
        nFusedA.push_back(ref_search_and_fuse_scene(*A, A->KFs[k], A->Siws[k], vReplacePts, 15.0, M1a, C));
        std::vector<std::pair<long, long> > r;
        for (std::map<mapPts *, mapPts *>::iterator it = vReplacePts.begin(); it != vReplacePts.end(); ++it) { r.push_back(std::make_pair((long)it->first->mnId, (long)it->second->mnId)); it->second->Replace(A->mpCurrentKF, it->first, M1a); }
        repA.push_back(r);
    }
    // ... and the adapter on B: one search before the loops, then the body per keyframe
    tsorb_adapter::FuseSceneSearch<keyframe> S; int redone = 0;
    if (tsorb_adapter::fuse_scene_search<Tr>(ctx, B->KFs, B->Siws, B->vLoopPts, B->mpMatchedKF, 15.0, S, on_host) != TSORB_OK) FAIL("fuse_scene_search failed");
    for (size_t k = 0; k < B->KFs.size(); k++) {
        std::map<mapPts *, mapPts *> vReplacePts;
        nFusedB.push_back(tsorb_adapter::search_and_fuse_scene<Tr>(B->KFs[k], S, B->vLoopPts, B->mpMatchedKF, B->mpCurrentKF, &B->Map, vReplacePts, TH_LOW, M1b, &redone));
        std::vector<std::pair<long, long> > r;
        for (std::map<mapPts *, mapPts *>::iterator it = vReplacePts.begin(); it != vReplacePts.end(); ++it) { r.push_back(std::make_pair((long)it->first->mnId, (long)it->second->mnId)); it->second->Replace(B->mpCurrentKF, it->first, M1b); }
        repB.push_back(r);
    }
    if (nFusedA != nFusedB) FAIL("nFused differs");
    if (repA != repB) FAIL("vReplacePts differs");
    if (M1a.adds != M1b.adds) FAIL("the covisibility updates differ");
    { std::vector<long> a, b; signature(*A, a); signature(*B, b); if (a != b) FAIL("the worlds differ after the run (observations added, replacements)"); }
    if (ctx) tsorb_destroy(ctx);
    FILE *f = fopen(outp, "wb"); if (!f) return 2;
    dump_call(f, "fuse_", S.call); dump_call(f, "more_", mms.call);
    fclose(f);
    long fused = 0; for (size_t k = 0; k < nFusedA.size(); k++) fused += nFusedA[k];
    printf("loop fuse from C++: ok mode=%s skipped=%ld source_changed=%ld added=%ld not_old=%ld neg_depth=%ld outside=%ld empty=%ld redone=%d fused=%ld queries=%d mm_queries=%d mm_matches=%ld mm_text=%ld mm_convert=%ld\n",
           on_host ? "host" : "device", C.skipped, C.source_changed, C.added, C.not_old, C.neg_depth, C.outside, C.empty, redone, fused, S.call.nq(), mms.call.nq(), mm_matches, mm_text, mm_convert);
    return 0;
}
