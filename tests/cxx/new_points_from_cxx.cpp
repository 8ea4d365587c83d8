// TEST DRIVER: the head of tracking::TrackNewKeyframe (SearchForTriangular + GetForTriangular) and tracking::SearchForInitializ from C++ -- adapter/tsorb_new_points.hpp's
// two bodies over mock types of this file.
// Usage: new_points_from_cxx [--host] <in.bin> <out.bin>
//   in : int32 mode (0: tracking, 1: initializer), n1, n2, Win; double K[4], Trw[16], Tcw[16], bounds[4] (mnMinX, mnMaxX, mnMinY, mnMaxY); frame 1: float pt[n1][2],
//        int32 octave[n1], uint8 desc[n1][32], int32 vMatches2D3D[n1], vTextObjInfo[n1]; frame 2: float kp6[n2][6], uint8 desc[n2][32], int32 vMatches2D3D[n2]
//   out: int32 rc, the returned count, n_new; int32 vMatchIdx12[n1]; double vNewpts[n_new][3]; int32 vNewptsMatch[n_new][2]
// --host touches no device and covers the search: the adapter's gather, the call replaced by a plain transcription of the chain over the gathered queries (its own grid
// and window walk), the scatter -- and the whole compared here with a plain transcription of the reference's loop over ALL features of frame 1 with the reference's own
// skip conditions: vMatchIdx12 and nMatches must be the same.  It triangulates nothing: n_new = 0 and the returned count is nMatches.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tsorb_new_points.hpp"

struct Vec3 { double v[3]; };
struct Mat33 { double m[9]; double operator()(int r, int c) const { return m[3*r + c]; } };
struct Mat44 { double m[16]; double operator()(int r, int c) const { return m[4*r + c]; } };
struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave; };
struct Descr { std::vector<uint8_t> d; };
struct Frame { int iN; std::vector<KeyPoint> vKeys; Descr mDescr; std::vector<int> vMatches2D3D, vTextObjInfo; Mat44 mTcw; Mat33 mK; double mnMinX, mnMaxX, mnMinY, mnMaxY; Frame() : iN(0) {} };
typedef std::pair<size_t, size_t> match;
struct Traits {
    static const uint8_t *row(const Descr &m, int i) { return m.d.data() + 32*(size_t)i; }
    static Vec3 vec3(double a, double b, double c) { Vec3 v; v.v[0] = a; v.v[1] = b; v.v[2] = c; return v; }
};

// ---- the plain transcription of the reference
#define FRAME_GRID_COLS 64
#define FRAME_GRID_ROWS 48
struct Grid { std::vector<size_t> cell[FRAME_GRID_COLS][FRAME_GRID_ROWS]; double iw, ih; };
static void AssignFeaturesToGrid(const Frame &F, Grid &G) {                                                            // frame.cc:372-407
    G.iw = (double)FRAME_GRID_COLS/(F.mnMaxX - F.mnMinX); G.ih = (double)FRAME_GRID_ROWS/(F.mnMaxY - F.mnMinY);
    for (int i = 0; i < F.iN; i++) { const int posX = (int)round(((double)F.vKeys[(size_t)i].pt.x - F.mnMinX)*G.iw), posY = (int)round(((double)F.vKeys[(size_t)i].pt.y - F.mnMinY)*G.ih);
        if (posX < 0 || posX >= FRAME_GRID_COLS || posY < 0 || posY >= FRAME_GRID_ROWS) continue;
        G.cell[posX][posY].push_back((size_t)i); }
}
static std::vector<size_t> GetFeaturesInArea(const Frame &F, const Grid &G, float x, float y, float r, int minLevel, int maxLevel) {      // frame.cc:415-468
    std::vector<size_t> vIndices;
    const int nMinCellX = std::max(0, (int)floor(((double)x - F.mnMinX - (double)r)*G.iw)); if (nMinCellX >= FRAME_GRID_COLS) return vIndices;
    const int nMaxCellX = std::min(FRAME_GRID_COLS - 1, (int)ceil(((double)x - F.mnMinX + (double)r)*G.iw)); if (nMaxCellX < 0) return vIndices;
    const int nMinCellY = std::max(0, (int)floor(((double)y - F.mnMinY - (double)r)*G.ih)); if (nMinCellY >= FRAME_GRID_ROWS) return vIndices;
    const int nMaxCellY = std::min(FRAME_GRID_ROWS - 1, (int)ceil(((double)y - F.mnMinY + (double)r)*G.ih)); if (nMaxCellY < 0) return vIndices;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++) for (int iy = nMinCellY; iy <= nMaxCellY; iy++) { const std::vector<size_t> &vCell = G.cell[ix][iy];
        for (size_t j = 0; j < vCell.size(); j++) { const KeyPoint &kpUn = F.vKeys[vCell[j]];
            if (bCheckLevels) { if (kpUn.octave < minLevel) continue; if (maxLevel >= 0) if (kpUn.octave > maxLevel) continue; }
            const float distx = kpUn.pt.x - x, disty = kpUn.pt.y - y;
            if (fabsf(distx) < r && fabsf(disty) < r) vIndices.push_back(vCell[j]); } }
    return vIndices;
}
static int DescriptorDistance(const uint8_t *a, const uint8_t *b) { int d = 0; for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k])); return d; }      // tracking.cc:2762-2778
// SearchForTriangular (init = false, :1347-1411) / SearchForInitializ (init = true, :1045-1109)
static int Search(const Frame &F1, const Frame &F2, const Grid &G, int Win, bool init, std::vector<int> &vMatchIdx12) {
    const int TH_LOW = 50; int nMatches = 0;
    vMatchIdx12 = std::vector<int>((size_t)F1.iN, -1);
    std::vector<int> vMatchDist((size_t)F2.iN, INT_MAX), vMatchIdx21((size_t)F2.iN, -1);
    for (size_t i1 = 0; i1 < (size_t)F1.iN; i1++) {
        if (init) { if (F1.vKeys[i1].octave > 0) continue; }
        else { if (F1.vMatches2D3D[i1] >= 0) continue; if (F1.vTextObjInfo[i1] >= 0) continue; }
        const KeyPoint Fea = F1.vKeys[i1]; const int PyrLevel1 = Fea.octave; const float ScaleORB = 1.2f; const float radius = init ? (float)Win : Win*ScaleORB;
        const std::vector<size_t> vF2Candidate = GetFeaturesInArea(F2, G, Fea.pt.x, Fea.pt.y, radius, PyrLevel1, PyrLevel1);
        if (vF2Candidate.empty()) continue;
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (size_t k = 0; k < vF2Candidate.size(); k++) { const size_t i2 = vF2Candidate[k];
            if (!init && F2.vMatches2D3D[i2] >= 0) continue;
            const int dist = DescriptorDistance(Traits::row(F1.mDescr, (int)i1), Traits::row(F2.mDescr, (int)i2));
            if (vMatchDist[i2] <= dist) continue;
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = (int)i2; } else if (dist < bestDist2) bestDist2 = dist; }
        if (bestDist <= TH_LOW) {
            if (init && !(bestDist < (double)bestDist2*0.9)) continue;
            if (vMatchIdx21[(size_t)bestIdx2] >= 0) { vMatchIdx12[(size_t)vMatchIdx21[(size_t)bestIdx2]] = -1; nMatches--; }
            vMatchIdx12[i1] = bestIdx2; vMatchIdx21[(size_t)bestIdx2] = (int)i1; vMatchDist[(size_t)bestIdx2] = bestDist; nMatches++; }
    }
    return nMatches;
}
// the call, transcribed: the chain over the gathered queries
static void chain_of(const tsorb_adapter::NewPointsCall &c, const Frame &F2, const Grid &G, int th_low, bool use_ratio, double ratio, std::vector<int32_t> &match12, int32_t &n_match) {
    const size_t Q = c.feat.size(); match12.assign(Q, -1); n_match = 0;
    std::vector<int> md((size_t)F2.iN, INT_MAX), own((size_t)F2.iN, -1);
    for (size_t q = 0; q < Q; q++) { const std::vector<size_t> cand = GetFeaturesInArea(F2, G, c.qxy[2*q], c.qxy[2*q + 1], c.qr[q], c.qlev[2*q], c.qlev[2*q + 1]);
        int best = INT_MAX, second = INT_MAX, bi = -1;
        for (size_t k = 0; k < cand.size(); k++) { const size_t i2 = cand[k]; if (!c.elig2.empty() && !c.elig2[i2]) continue;
            const int d = DescriptorDistance(&c.qdesc[32*q], Traits::row(F2.mDescr, (int)i2)); if (md[i2] <= d) continue;
            if (d < best) { second = best; best = d; bi = (int)i2; } else if (d < second) second = d; }
        if (!(best <= th_low && (!use_ratio || (double)best < (double)second*ratio))) continue;
        if (own[(size_t)bi] >= 0) { match12[(size_t)own[(size_t)bi]] = -1; n_match--; }
        match12[q] = bi; own[(size_t)bi] = (int)q; md[(size_t)bi] = best; n_match++; }
}

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "new_points_from_cxx: %s\n", msg); return 1; } while (0)

int main(int argc, char **argv) {
    const bool host = argc > 1 && strcmp(argv[1], "--host") == 0;
    if (argc != (host ? 4 : 3)) FAIL("usage: new_points_from_cxx [--host] in.bin out.bin");
    FILE *f = fopen(argv[host ? 2 : 1], "rb"); if (!f) FAIL("cannot open input");
    int32_t hd[4]; double K[4], bounds[4]; Frame F1, F2;
    if (!rd(f, hd, 4) || !rd(f, K, 4) || !rd(f, F1.mTcw.m, 16) || !rd(f, F2.mTcw.m, 16) || !rd(f, bounds, 4) || hd[0] < 0 || hd[0] > 1 || hd[1] < 0 || hd[2] < 0) FAIL("bad header");
    const int mode = hd[0], n1 = hd[1], n2 = hd[2], Win = hd[3];
    const double k9[9] = { K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1 }; for (int i = 0; i < 9; i++) F1.mK.m[i] = F2.mK.m[i] = k9[i];
    F1.mnMinX = F2.mnMinX = bounds[0]; F1.mnMaxX = F2.mnMaxX = bounds[1]; F1.mnMinY = F2.mnMinY = bounds[2]; F1.mnMaxY = F2.mnMaxY = bounds[3];
    std::vector<float> px(2*(size_t)n1), kp6(6*(size_t)n2); std::vector<int32_t> oct((size_t)n1), m3d((size_t)n1), tobj((size_t)n1), m3d2((size_t)n2);
    F1.mDescr.d.resize(32*(size_t)n1); F2.mDescr.d.resize(32*(size_t)n2);
    if (!rd(f, px.data(), px.size()) || !rd(f, oct.data(), oct.size()) || !rd(f, F1.mDescr.d.data(), F1.mDescr.d.size()) || !rd(f, m3d.data(), m3d.size()) || !rd(f, tobj.data(), tobj.size()) ||
        !rd(f, kp6.data(), kp6.size()) || !rd(f, F2.mDescr.d.data(), F2.mDescr.d.size()) || !rd(f, m3d2.data(), m3d2.size())) FAIL("short input");
    fclose(f);
    F1.iN = n1; F2.iN = n2;
    for (int i = 0; i < n1; i++) { const KeyPoint k = { { px[2*(size_t)i], px[2*(size_t)i + 1] }, 31.f, 0.f, 0.f, oct[(size_t)i] }; F1.vKeys.push_back(k);
        F1.vMatches2D3D.push_back(m3d[(size_t)i]); F1.vTextObjInfo.push_back(tobj[(size_t)i]); }
    for (int i = 0; i < n2; i++) { const float *p = &kp6[6*(size_t)i]; const KeyPoint k = { { p[0], p[1] }, p[2], p[3], p[4], (int)p[5] }; F2.vKeys.push_back(k);
        F2.vMatches2D3D.push_back(m3d2[(size_t)i]); F2.vTextObjInfo.push_back(-1); }
    std::vector<int> vMatchIdx12; std::vector<Vec3> vNewpts; std::vector<match> vNewptsMatch; void *ctx = 0; int ret = 0, rc = 0;
    if (host) {
        Grid *G = new Grid; AssignFeaturesToGrid(F2, *G);
        tsorb_adapter::NewPointsCall c;
        if (mode == 0) tsorb_adapter::gather_triangular_queries<Traits>(&F1, F2, Win, c); else tsorb_adapter::gather_initializ_queries<Traits>(F1, Win, c);
        chain_of(c, F2, *G, 50, mode == 1, 0.9, c.match12, c.n_match);
        tsorb_adapter::scatter_matches(c, (size_t)F1.iN, vMatchIdx12); ret = c.n_match;
        std::vector<int> ref; const int nMatches = Search(F1, F2, *G, Win, mode == 1, ref);
        delete G;
        if (ref != vMatchIdx12 || nMatches != ret) FAIL("vMatchIdx12 differs from the reference's loop");
    } else {
        if (tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0) != TSORB_OK) FAIL("tsorb_create");
        ret = mode == 0 ? tsorb_adapter::search_for_triangular_and_get<Traits>(ctx, &F1, F2, Win, vMatchIdx12, vNewpts, vNewptsMatch)
                        : tsorb_adapter::search_for_initializ<Traits>(ctx, F1, F2, Win, vMatchIdx12);
        if (ret < 0) { fprintf(stderr, "the call failed: %s\n", tsorb_last_error(ctx)); return 1; }
    }
    if ((int)vMatchIdx12.size() != n1 || vNewpts.size() != vNewptsMatch.size()) FAIL("the vectors have another length");
    const int32_t rc32 = rc, ret32 = ret, n_new = (int32_t)vNewpts.size();
    FILE *g = fopen(argv[host ? 3 : 2], "wb"); if (!g) FAIL("cannot open output");
    wr(g, &rc32, 1); wr(g, &ret32, 1); wr(g, &n_new, 1);
    for (int i = 0; i < n1; i++) { const int32_t m = vMatchIdx12[(size_t)i]; wr(g, &m, 1); }
    for (size_t i = 0; i < vNewpts.size(); i++) wr(g, vNewpts[i].v, 3);
    for (size_t i = 0; i < vNewptsMatch.size(); i++) { const int32_t p[2] = { (int32_t)vNewptsMatch[i].first, (int32_t)vNewptsMatch[i].second }; wr(g, p, 2); }
    fclose(g);
    if (ctx) tsorb_destroy(ctx);
    printf(host ? "new points from C++ (host): ok\n" : "new points from C++: ok\n");
    return 0;
}
