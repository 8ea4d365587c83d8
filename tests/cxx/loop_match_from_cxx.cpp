// TEST INFRASTRUCTURE: loopClosing::SearchMatch's two matchers through the adapter (adapter/tsorb_loop_match.hpp) from C++, over mock types of its own.
//
//   loop_match_from_cxx <in.bin> <out.bin>      the mock world of tests/loop_match_world.py (formats there) through search_match_text and search_match_other;
//                                               exit code 0 and "loop match from C++: ok" = both ran and the outputs are consistent
//   loop_match_from_cxx --time [reps]           tools/diag/gpu_loop_match.py: the time of a call (copies included) at the shapes of profiles/loop_match_timing.txt
//                                               beside a single-thread transcription of the same loops on the host
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "tsorb_loop_match.hpp"

namespace lm {
struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } };
struct Mat { int rows, cols; std::vector<uint8_t> data; Mat() : rows(0), cols(32) {} };                  // cv::Mat CV_8U, 32 columns
struct KeyPoint { struct Pt { float x, y; } pt; };
struct keyframe; struct mapText;
struct TextObservation { mapText *obj; std::vector<int> idx; };
struct keyframe {
    Mat FrameImg;                                                                                        // (rows, cols only)
    std::vector<KeyPoint> vKeys; Mat mDescr; std::vector<int> vTextObjInfo, vMatches2D3D, vTextDeteCorMap;
    std::vector<std::vector<Vec2> > vTextDete; std::vector<std::vector<KeyPoint> > vKeysText; std::vector<Mat> mDescrText;
    std::vector<TextObservation *> vObvText;
};
struct mapText {
    std::vector<std::pair<keyframe *, std::vector<int> > > obs;
    bool GetObvIdx(keyframe *KF, std::vector<int> &idx) const { for (size_t i = 0; i < obs.size(); i++) if (obs[i].first == KF) { idx = obs[i].second; return true; } return false; }
};
struct MatchmapTextRes { mapText *mapObj; };
struct Tr { static int rows(const Mat &m) { return m.rows; } static const uint8_t *row(const Mat &m, int i) { return m.data.data() + 32*(size_t)i; } };
}  // namespace lm

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool rd_i(FILE *f, int32_t &v) { return rd(f, &v, 4); }
static bool rd_vec(FILE *f, std::vector<int> &v, int n) { v.resize((size_t)n); return rd(f, v.data(), 4*(size_t)n); }

// ---- the host loops, transcribed (single thread): what the device calls replace
static inline int hamming(const uint8_t *a, const uint8_t *b) {
    const uint32_t *pa = (const uint32_t *)a, *pb = (const uint32_t *)b; int d = 0;
    for (int i = 0; i < 8; i++) d += __builtin_popcount(pa[i] ^ pb[i]);
    return d;
}
static int host_scan(int n1, const uint8_t *d1, const uint8_t *e1, int n2, const uint8_t *d2, const uint8_t *e2, int th_low, double ratio, std::vector<int> &m12) {
    m12.assign((size_t)n1, -1); std::vector<int> md((size_t)n2, INT_MAX), m21((size_t)n2, -1);
    int nMatches = 0;
    for (int i1 = 0; i1 < n1; i1++) {
        if (!e1[i1]) continue;
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (int i2 = 0; i2 < n2; i2++) {
            if (!e2[i2]) continue;
            const int dist = hamming(d1 + 32*(size_t)i1, d2 + 32*(size_t)i2);
            if (md[(size_t)i2] <= dist) continue;
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; } else if (dist < bestDist2) bestDist2 = dist;
        }
        if (bestDist <= th_low && bestDist < (double)bestDist2*ratio) {
            if (m21[(size_t)bestIdx2] >= 0) { m12[(size_t)m21[(size_t)bestIdx2]] = -1; nMatches--; }
            m12[(size_t)i1] = bestIdx2; m21[(size_t)bestIdx2] = i1; md[(size_t)bestIdx2] = bestDist; nMatches++;
        }
    }
    return nMatches;
}
static int host_text(int n1, const uint8_t *d1, int n2, const uint8_t *d2, std::vector<int> &train, std::vector<int> &dist) {
    train.assign((size_t)n1, -1); dist.assign((size_t)n1, INT_MAX); int good = 0; double min_dist = 10000;
    for (int q = 0; q < n1; q++) { for (int j = 0; j < n2; j++) { const int d = hamming(d1 + 32*(size_t)q, d2 + 32*(size_t)j); if (d < dist[(size_t)q]) { dist[(size_t)q] = d; train[(size_t)q] = j; } }
        if (dist[(size_t)q] < min_dist) min_dist = dist[(size_t)q]; }
    for (int q = 0; q < n1; q++) if (dist[(size_t)q] < (2*min_dist > 30.0 ? 2*min_dist : 30.0)) good++;
    return good;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state*1664525u + 1013904223u; return rng_state >> 8; }
static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

static int time_mode(int reps) {
    void *ctx = 0;
    if (tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0) != TSORB_OK) { fprintf(stderr, "tsorb_create failed\n"); return 1; }
    const int n = 1000, w = 640, h = 480;
    // a current keyframe and eight candidates: the current descriptors with up to 60 bits flipped, 80 % with 3-D information, two boxes per image
    std::vector<uint8_t> d1(32*(size_t)n), h1((size_t)n), d2(8*32*(size_t)n), h2(8*(size_t)n); std::vector<float> xy1(2*(size_t)n), xy2(8*2*(size_t)n);
    for (size_t i = 0; i < d1.size(); i++) d1[i] = (uint8_t)rnd();
    for (int i = 0; i < n; i++) { h1[(size_t)i] = rnd() % 5 != 0; xy1[2*(size_t)i] = (float)(rnd() % 6390)/10.f; xy1[2*(size_t)i + 1] = (float)(rnd() % 4790)/10.f; }
    for (int c = 0; c < 8; c++) for (int i = 0; i < n; i++) { const size_t r = (size_t)c*n + i, s = (size_t)((i*7 + c*13) % n);
        memcpy(&d2[32*r], &d1[32*s], 32); const int nb = (int)(rnd() % 61); for (int b = 0; b < nb; b++) { const uint32_t k = rnd() % 256; d2[32*r + (k >> 3)] ^= (uint8_t)(1u << (k & 7)); }
        h2[r] = rnd() % 5 != 0; xy2[2*r] = (float)(rnd() % 6390)/10.f; xy2[2*r + 1] = (float)(rnd() % 4790)/10.f; }
    std::vector<int32_t> off2(9), qoff(9); std::vector<double> qc, qn;
    for (int c = 0; c <= 8; c++) { off2[(size_t)c] = c*n; qoff[(size_t)c] = 2*c; }
    for (int b = 0; b < 16; b++) { const double x = 40 + 30*b, y = 30 + 20*b; const double q[8] = { x, y, x + 90, y + 4, x + 88, y + 40, x - 3, y + 37 };
        qc.insert(qc.end(), q, q + 8); for (int k = 0; k < 8; k++) qn.push_back(q[k] + 11); }
    std::vector<int32_t> m12(8*(size_t)n), nm(8);
    printf("# per call, copies included; device = the median of %d calls after a warm-up, host = a single-thread transcription of the reference's loops (this binary, g++ -O2)\n", reps);
    printf("# call                          shape                         device_ms   host_ms   host/device\n");
    const int ncs[3] = { 1, 4, 8 };
    for (int k = 0; k < 3; k++) {
        const int nc = ncs[k]; std::vector<double> t;
        for (int r = 0; r < reps + 2; r++) { const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            const int rc = tsorb_match_brute_scene(ctx, w, h, n, xy1.data(), d1.data(), h1.data(), nc, off2.data(), xy2.data(), d2.data(), h2.data(), qoff.data(), qc.data(), qn.data(), 50, 0.9, m12.data(), nm.data());
            if (rc != TSORB_OK) { fprintf(stderr, "scene: %d (%s)\n", rc, tsorb_last_error(ctx)); return 1; }
            if (r >= 2) t.push_back(ms_since(t0)); }
        std::sort(t.begin(), t.end());
        // the host side: eligibility by has3d only (the label images are a cv::fillPoly and two reads per feature there; not transcribed), then the scan
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); long total = 0; std::vector<int> hm;
        for (int c = 0; c < nc; c++) total += host_scan(n, d1.data(), h1.data(), n, &d2[32*(size_t)c*n], &h2[(size_t)c*n], 50, 0.9, hm);
        const double th = ms_since(t0);
        printf("tsorb_match_brute_scene         1000 x 1000, %d candidate(s)   %9.3f %9.3f %9.1f     (matches: device %d for the last candidate, host total %ld)\n", nc, t[t.size()/2], th, th/t[t.size()/2], nm[(size_t)nc - 1], total);
    }
    const int nps[2] = { 8, 32 };
    for (int k = 0; k < 2; k++) {
        const int np = nps[k]; std::vector<int32_t> o1((size_t)np + 1), o2((size_t)np + 1); for (int p = 0; p <= np; p++) o1[(size_t)p] = o2[(size_t)p] = 60*p;
        std::vector<int32_t> tr(60*(size_t)np), di(60*(size_t)np); std::vector<uint8_t> gd(60*(size_t)np), a(32*60*(size_t)np), b(32*60*(size_t)np);
        for (size_t i = 0; i < a.size(); i++) { a[i] = d1[i % d1.size()]; b[i] = d2[i % d2.size()]; }
        std::vector<double> t;
        for (int r = 0; r < reps + 2; r++) { const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
            const int rc = tsorb_match_brute_text(ctx, np, o1.data(), a.data(), o2.data(), b.data(), tr.data(), di.data(), gd.data());
            if (rc != TSORB_OK) { fprintf(stderr, "text: %d (%s)\n", rc, tsorb_last_error(ctx)); return 1; }
            if (r >= 2) t.push_back(ms_since(t0)); }
        std::sort(t.begin(), t.end());
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); long good = 0; std::vector<int> ht, hd;
        for (int p = 0; p < np; p++) good += host_text(60, &a[32*60*(size_t)p], 60, &b[32*60*(size_t)p], ht, hd);
        const double th = ms_since(t0);
        long dev_good = 0; for (size_t i = 0; i < gd.size(); i++) dev_good += gd[i];
        printf("tsorb_match_brute_text          %2d pairs of 60 x 60            %9.3f %9.3f %9.1f     (good: device %ld, host %ld)\n", np, t[t.size()/2], th, th/t[t.size()/2], dev_good, good);
    }
    tsorb_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && strcmp(argv[1], "--time") == 0) return time_mode(argc >= 3 ? atoi(argv[2]) : 20);
    if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin | --time [reps]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int32_t hd[4];
    if (!rd(f, hd, 16) || hd[2] < 1 || hd[3] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int n_kf = hd[2], n_obj = hd[3];
    std::vector<lm::keyframe> kfs((size_t)n_kf); std::vector<lm::mapText> objs((size_t)n_obj);
    bool ok = true;
    for (int k = 0; k < n_kf && ok; k++) {
        lm::keyframe &K = kfs[(size_t)k]; K.FrameImg.cols = hd[0]; K.FrameImg.rows = hd[1];
        int32_t n = 0, nd = 0; ok = rd_i(f, n) && n >= 0; if (!ok) break;
        std::vector<float> xy(2*(size_t)n); K.mDescr.rows = n; K.mDescr.data.resize(32*(size_t)n);
        ok = rd(f, xy.data(), 8*(size_t)n) && rd(f, K.mDescr.data.data(), 32*(size_t)n) && rd_vec(f, K.vTextObjInfo, n) && rd_vec(f, K.vMatches2D3D, n) && rd_i(f, nd) && nd >= 0 && rd_vec(f, K.vTextDeteCorMap, nd);
        if (!ok) break;
        K.vKeys.resize((size_t)n); for (int i = 0; i < n; i++) { K.vKeys[(size_t)i].pt.x = xy[2*(size_t)i]; K.vKeys[(size_t)i].pt.y = xy[2*(size_t)i + 1]; }
        K.vTextDete.resize((size_t)nd); K.vKeysText.resize((size_t)nd); K.mDescrText.resize((size_t)nd);
        for (int d = 0; d < nd && ok; d++) { double q[8]; int32_t rows = 0; ok = rd(f, q, 64) && rd_i(f, rows) && rows >= 0; if (!ok) break;
            for (int c = 0; c < 4; c++) { lm::Vec2 v; v.v[0] = q[2*c]; v.v[1] = q[2*c + 1]; K.vTextDete[(size_t)d].push_back(v); }
            K.vKeysText[(size_t)d].resize((size_t)rows); K.mDescrText[(size_t)d].rows = rows; K.mDescrText[(size_t)d].data.resize(32*(size_t)rows); ok = rd(f, K.mDescrText[(size_t)d].data.data(), 32*(size_t)rows); }
    }
    for (int o = 0; o < n_obj && ok; o++) { int32_t no = 0; ok = rd_i(f, no) && no >= 0;
        for (int j = 0; j < no && ok; j++) { int32_t k = 0, ni = 0; std::vector<int> idx; ok = rd_i(f, k) && rd_i(f, ni) && k >= 0 && k < n_kf && ni >= 0 && rd_vec(f, idx, ni);
            if (ok) objs[(size_t)o].obs.push_back(std::make_pair(&kfs[(size_t)k], idx)); } }
    int32_t n_obv = 0; ok = ok && rd_i(f, n_obv) && n_obv >= 0;
    std::vector<lm::TextObservation> obv((size_t)(ok ? n_obv : 0)); std::vector<std::vector<lm::MatchmapTextRes> > vMatchTexts((size_t)(ok ? n_obv : 0));
    for (int j = 0; j < n_obv && ok; j++) { int32_t o = 0, ni = 0; ok = rd_i(f, o) && rd_i(f, ni) && o >= 0 && o < n_obj && ni >= 0 && rd_vec(f, obv[(size_t)j].idx, ni); if (ok) obv[(size_t)j].obj = &objs[(size_t)o]; }
    for (int j = 0; j < n_obv && ok; j++) { int32_t nr = 0; ok = rd_i(f, nr) && nr >= 0;
        for (int r = 0; r < nr && ok; r++) { int32_t o = 0; ok = rd_i(f, o) && o >= 0 && o < n_obj; if (ok) { lm::MatchmapTextRes m; m.mapObj = &objs[(size_t)o]; vMatchTexts[(size_t)j].push_back(m); } } }
    fclose(f);
    if (!ok) { fprintf(stderr, "input incomplete\n"); return 2; }
    lm::keyframe *Cur = &kfs[0];
    for (size_t j = 0; j < obv.size(); j++) Cur->vObvText.push_back(&obv[j]);
    std::vector<lm::keyframe *> cands; for (int k = 1; k < n_kf; k++) cands.push_back(&kfs[(size_t)k]);

    void *ctx = 0;
    int rc = tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0);
    if (rc != TSORB_OK) { fprintf(stderr, "tsorb_create: %d\n", rc); return 1; }
    std::vector<tsorb_adapter::CandidateTextMatch> text;
    rc = tsorb_adapter::search_match_text<lm::Tr>(ctx, Cur, cands, vMatchTexts, text);
    if (rc != TSORB_OK) { fprintf(stderr, "search_match_text: %d (%s)\n", rc, tsorb_last_error(ctx)); return 1; }
    std::vector<std::vector<int> > vMatchIdx12; std::vector<int> nMatches;
    rc = tsorb_adapter::search_match_other<lm::Tr>(ctx, Cur, cands, text, vMatchIdx12, nMatches);
    if (rc != TSORB_OK) { fprintf(stderr, "search_match_other: %d (%s)\n", rc, tsorb_last_error(ctx)); return 1; }
    // consistency: per candidate alone = its part of the one call; the counts are the rows' entries >= 0; a text match's indices are inside its pair
    size_t n_pairs = 0, n_good = 0; long n_scene = 0;
    for (size_t ic = 0; ic < cands.size(); ic++) {
        std::vector<lm::keyframe *> one(1, cands[ic]); std::vector<tsorb_adapter::CandidateTextMatch> t1; std::vector<std::vector<int> > m1; std::vector<int> n1;
        if (tsorb_adapter::search_match_text<lm::Tr>(ctx, Cur, one, vMatchTexts, t1) != TSORB_OK || tsorb_adapter::search_match_other<lm::Tr>(ctx, Cur, one, t1, m1, n1) != TSORB_OK) { fprintf(stderr, "candidate %zu alone failed\n", ic); return 1; }
        if (m1[0] != vMatchIdx12[ic] || n1[0] != nMatches[ic] || t1[0].pairs.size() != text[ic].pairs.size() || t1[0].quad_cur != text[ic].quad_cur) { fprintf(stderr, "candidate %zu differs between the one call and its own\n", ic); return 1; }
        int cnt = 0; for (size_t i = 0; i < vMatchIdx12[ic].size(); i++) cnt += vMatchIdx12[ic][i] >= 0;
        if (cnt != nMatches[ic]) { fprintf(stderr, "candidate %zu: nMatches %d, %d entries\n", ic, nMatches[ic], cnt); return 1; }
        n_scene += cnt;
        for (size_t p = 0; p < text[ic].pairs.size(); p++) { const tsorb_adapter::TextPairMatch &P = text[ic].pairs[p]; n_pairs++; n_good += P.match12.size();
            if (t1[0].pairs[p].match12.size() != P.match12.size()) { fprintf(stderr, "candidate %zu pair %zu differs\n", ic, p); return 1; }
            for (size_t g = 0; g < P.match12.size(); g++) if (P.match12[g].queryIdx < 0 || P.match12[g].queryIdx >= Cur->mDescrText[(size_t)P.idxCur].rows || P.match12[g].trainIdx < 0 || P.match12[g].trainIdx >= cands[ic]->mDescrText[(size_t)P.idxCan].rows) { fprintf(stderr, "match outside its pair\n"); return 1; } }
    }
    tsorb_destroy(ctx);
    FILE *o = fopen(argv[2], "wb"); if (!o) return 2;
    for (size_t ic = 0; ic < cands.size(); ic++) {
        int32_t v = (int32_t)text[ic].pairs.size(); fwrite(&v, 4, 1, o);
        for (size_t p = 0; p < text[ic].pairs.size(); p++) { const tsorb_adapter::TextPairMatch &P = text[ic].pairs[p];
            const int32_t h5[5] = { P.iObvText, P.iMatchRes, P.idxCur, P.idxCan, (int32_t)P.match12.size() }; fwrite(h5, 4, 5, o);
            for (size_t g = 0; g < P.match12.size(); g++) { const int32_t qt[2] = { P.match12[g].queryIdx, P.match12[g].trainIdx }; fwrite(qt, 4, 2, o); fwrite(&P.match12[g].distance, 4, 1, o); } }
        v = (int32_t)(text[ic].quad_cur.size()/8); fwrite(&v, 4, 1, o);
        if (v) { fwrite(text[ic].quad_cur.data(), 8, text[ic].quad_cur.size(), o); fwrite(text[ic].quad_can.data(), 8, text[ic].quad_can.size(), o); }
        v = (int32_t)vMatchIdx12[ic].size(); fwrite(&v, 4, 1, o);
        if (v) fwrite(vMatchIdx12[ic].data(), 4, vMatchIdx12[ic].size(), o);
        v = nMatches[ic]; fwrite(&v, 4, 1, o);
    }
    fclose(o);
    printf("loop match from C++: ok (%zu candidates, %zu text pairs, %zu good text matches, %ld scene matches)\n", cands.size(), n_pairs, n_good, n_scene);
    return 0;
}
