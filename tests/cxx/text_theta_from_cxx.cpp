// TEST DRIVER: tracking::InitialTextObjs / initializer::InitialTextObjs from C++ -- adapter/tsorb_text_theta.hpp's two bodies over mock types of this file.
// Usage: text_theta_from_cxx [--host] <in.bin> <out.bin>
//   in : int32 mode (0: tracking, 1: initializer), max_iterations, n_det; uint32 seed; double K[4], Trw[16], Tcw[16]; per detection: int32 cormap, n; float host[n][2],
//        targ[n][2]; double rho[n] (the initializer's TextKeys3D(2); for --host in tracking mode the rho to use where the device would triangulate)
//   out: int32 rc, n_plane, N, H; int32 det[n_plane], off[n_plane+1], hyp_off[n_plane+1], triple[H][3]; float host_xy[N][2], targ_xy[N][2]; double rho[N] (given, or the
//        call's rho_out), Tcr[12], K[4]; int32 sel[n_plane]; double theta[n_plane][3], score[n_plane]; int32 nobj; double mNcr[nobj][3]; uint8 vNGOOD[nobj]
// --host touches no device: the adapter's gather and draws, the call replaced by a plain transcription of SolveTheta over the gathered arrays, the scatter -- and the
// whole compared here with a plain transcription of the reference's loops (its own draws from the same seed, its own vectors): mNcr and vNGOOD must be the same bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tsorb_text_theta.hpp"

struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat33 { double m[9]; double operator()(int r, int c) const { return m[3*r + c]; } };
struct Mat44 { double m[16]; double operator()(int r, int c) const { return m[4*r + c]; } double &operator()(int r, int c) { return m[4*r + c]; } };
struct Point2f { float x, y; };
struct Frame { Mat44 mTcw; Mat33 mK; double fx, fy, cx, cy; int iNTextObj; std::vector<Vec3> mNcr; std::vector<bool> vNGOOD; std::vector<int> vTextDeteCorMap;
    std::vector<std::vector<Point2f> > vKeysNewTextTrack, vKeysTextTrack; Frame() : iNTextObj(0) {} };

static uint32_t g_lcg = 1u; static int g_seeded = 0;
static Mat44 rigid_inverse(const Mat44 &T) { Mat44 o; for (int i = 0; i < 16; i++) o.m[i] = i == 15 ? 1.0 : 0.0;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o(r, c) = T(c, r); o(r, 3) = -((T(0, r)*T(0, 3) + T(1, r)*T(1, 3)) + T(2, r)*T(2, 3)); }
    return o; }
struct Traits {
    static int random_int(int lo, int hi) { g_lcg = g_lcg*1664525u + 1013904223u; return lo + (int)((g_lcg >> 8) % (uint32_t)(hi - lo + 1)); }
    static void seed_rand_once() { g_seeded++; }
    static void tcr_of(const Mat44 &Tcw, const Mat44 &Trw, double out[12]) { const Mat44 I = rigid_inverse(Trw);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) out[4*r + c] = ((Tcw(r, 0)*I(0, c) + Tcw(r, 1)*I(1, c)) + Tcw(r, 2)*I(2, c)) + Tcw(r, 3)*I(3, c); }
    static Vec3 vec3(double a, double b, double c) { Vec3 v; v(0) = a; v(1) = b; v(2) = c; return v; }
};

// ---- the plain transcription of the reference
static bool GetRANSACIdx(int MaxIterations, int SelectNum, int number, std::vector<std::vector<size_t> > &IdxOut) {                 // tool.cc:1366-1390
    if (number < 3) return false;
    IdxOut = std::vector<std::vector<size_t> >((size_t)MaxIterations, std::vector<size_t>((size_t)SelectNum, 0));
    for (int it = 0; it < MaxIterations; it++) { std::vector<size_t> vAvailableIndices; for (int i = 0; i < number; i++) vAvailableIndices.push_back((size_t)i);
        for (int j = 0; j < SelectNum; j++) { const int randi = Traits::random_int(0, (int)vAvailableIndices.size() - 1);
            IdxOut[(size_t)it][(size_t)j] = vAvailableIndices[(size_t)randi]; vAvailableIndices[(size_t)randi] = vAvailableIndices.back(); vAvailableIndices.pop_back(); } }
    return true;
}
static double SolveTheta(const size_t Idx[3], const double Tcr[12], const std::vector<Point2f> &Targfeat, const std::vector<Vec3> &HostRay, const double K[4], Vec3 &theta) {      // tracking.cc:1870-1917
    const float th = 5.991f;
    const Vec3 m1 = HostRay[Idx[0]], m2 = HostRay[Idx[1]], m3 = HostRay[Idx[2]];
    const double A = m3(1)/m3(0), B = 1.0/m3(0), C = (1 - m2(0)*B)/(m2(1) - m2(0)*A), D = (A*C - B)*m1(0) - C*m1(1) + 1, rho3pie = m3(2)/m3(0);
    const double rho2pie = (m2(2) - rho3pie*m2(0))/(m2(1) - m2(0)*A), rho1pie = m1(2) - rho3pie*m1(0) - rho2pie*(m1(1) - A*m1(0));
    theta(2) = rho1pie/D; theta(1) = rho2pie - C*theta(2); theta(0) = rho3pie - A*theta(1) - B*theta(2);
    double score = 0;
    for (size_t ipts = 0; ipts < HostRay.size(); ipts++) { const double m[3] = { HostRay[ipts](0), HostRay[ipts](1), 1.0 };
        const double rhoPred = m[0]*theta(0) + m[1]*theta(1) + m[2]*theta(2), s = 1.0/rhoPred; double P3d[3];
        for (int r = 0; r < 3; r++) P3d[r] = (Tcr[4*r]*m[0] + Tcr[4*r + 1]*m[1] + Tcr[4*r + 2]*m[2])*s + Tcr[4*r + 3];
        const double u = P3d[0]/P3d[2]*K[0] + K[2], v = P3d[1]/P3d[2]*K[1] + K[3], erroru = Targfeat[ipts].x - u, errorv = Targfeat[ipts].y - v, chiSquare2 = erroru*erroru + errorv*errorv;
        if (chiSquare2 > th) continue; else score += th - chiSquare2; }
    for (int k = 0; k < 3; k++) theta(k) = -theta(k);
    return score;
}
// GetTextTheta from step 5 on (:1700-1733) / the loop of initializer::InitialTextObjs (:159-180) over one detection with its rho; zero_triples: the initializer's plane of 3
static bool theta_of(const std::vector<Point2f> &Hostfeat, const std::vector<Point2f> &Targfeat, const std::vector<double> &vRho, const double Tcr[12], const double K[4],
                     int iMaxIterations, bool draw, Vec3 &theta) {
    std::vector<Vec3> vHostRayRho;
    for (size_t i = 0; i < Hostfeat.size(); i++) vHostRayRho.push_back(Traits::vec3(((double)Hostfeat[i].x - K[2])/K[0], ((double)Hostfeat[i].y - K[3])/K[1], vRho[i]));
    std::vector<std::vector<size_t> > RansacIdx((size_t)iMaxIterations, std::vector<size_t>(3, 0));
    if (draw && !GetRANSACIdx(iMaxIterations, 3, (int)Hostfeat.size(), RansacIdx)) return false;
    double BestScore = -1.0; Vec3 BestTheta = Traits::vec3(-1.0, -1.0, -1.0);
    for (size_t i0 = 0; i0 < RansacIdx.size(); i0++) { Vec3 thetaObj; const size_t Idx[3] = { RansacIdx[i0][0], RansacIdx[i0][1], RansacIdx[i0][2] };
        const double score = SolveTheta(Idx, Tcr, Targfeat, vHostRayRho, K, thetaObj);
        if (BestScore < score) { BestTheta = thetaObj; BestScore = score; } }
    if (BestScore < 0) return false;                                      // tracking: BestScore != -1; the scores are never negative
    theta = BestTheta;
    return true;
}

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "text_theta_from_cxx: %s\n", msg); return 1; } while (0)

int main(int argc, char **argv) {
    const bool host = argc > 1 && strcmp(argv[1], "--host") == 0;
    if (argc != (host ? 4 : 3)) FAIL("usage: text_theta_from_cxx [--host] in.bin out.bin");
    FILE *f = fopen(argv[host ? 2 : 1], "rb"); if (!f) FAIL("cannot open input");
    int32_t mode = 0, max_it = 0, nd = 0; uint32_t seed = 0; double K[4]; Mat44 Trw, Tcw;
    if (!rd(f, &mode, 1) || !rd(f, &max_it, 1) || !rd(f, &nd, 1) || !rd(f, &seed, 1) || !rd(f, K, 4) || !rd(f, Trw.m, 16) || !rd(f, Tcw.m, 16) || mode < 0 || mode > 1 || max_it < 1 || nd < 0)
        FAIL("bad header");
    Frame F1, F2; F1.mTcw = Trw; F2.mTcw = Tcw; F1.iNTextObj = nd;
    const double k9[9] = { K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1 }; for (int i = 0; i < 9; i++) F2.mK.m[i] = k9[i];
    F1.fx = K[0]; F1.fy = K[1]; F1.cx = K[2]; F1.cy = K[3];
    std::vector<std::vector<double> > rho((size_t)nd); std::vector<std::vector<Vec2> > TextKeys1((size_t)nd), TextKeys2((size_t)nd); std::vector<std::vector<Vec3> > TextKeys3D((size_t)nd);
    F1.vKeysNewTextTrack.resize((size_t)nd); F2.vKeysTextTrack.resize((size_t)nd);
    for (int d = 0; d < nd; d++) { int32_t cor = 0, n = 0; if (!rd(f, &cor, 1) || !rd(f, &n, 1) || n < 0) FAIL("short input");
        std::vector<float> h(2*(size_t)n), t(2*(size_t)n); rho[(size_t)d].resize((size_t)n);
        if (!rd(f, h.data(), h.size()) || !rd(f, t.data(), t.size()) || !rd(f, rho[(size_t)d].data(), (size_t)n)) FAIL("short input");
        F1.vTextDeteCorMap.push_back(cor);
        for (int i = 0; i < n; i++) { const Point2f a = { h[2*(size_t)i], h[2*(size_t)i + 1] }, b = { t[2*(size_t)i], t[2*(size_t)i + 1] };
            F1.vKeysNewTextTrack[(size_t)d].push_back(a); F2.vKeysTextTrack[(size_t)d].push_back(b);
            const Vec2 k1 = { { a.x, a.y } }, k2 = { { b.x, b.y } }; TextKeys1[(size_t)d].push_back(k1); TextKeys2[(size_t)d].push_back(k2);
            TextKeys3D[(size_t)d].push_back(Traits::vec3(((double)a.x - K[2])/K[0], ((double)a.y - K[3])/K[1], rho[(size_t)d][(size_t)i])); } }
    fclose(f);
    tsorb_adapter::TextThetaCall c; void *ctx = 0; int rc = 0;
    g_lcg = seed;
    if (host) {
        if (mode == 0) tsorb_adapter::gather_text_objs<Traits>(&F1, F2, c, max_it); else tsorb_adapter::gather_text_objs_init<Traits>(&F1, &F2, TextKeys1, TextKeys3D, TextKeys2, max_it, c);
        const size_t P = c.det.size();
        c.sel.assign(P, -1); c.theta.assign(3*P, 0.0); c.score.assign(P, 0.0); c.rho_out.clear();
        for (size_t k = 0; k < P; k++) for (int i = c.off[k]; i < c.off[k + 1]; i++) c.rho_out.push_back(mode == 1 ? c.rho[(size_t)i] : rho[(size_t)c.det[k]][(size_t)(i - c.off[k])]);
        for (size_t k = 0; k < P; k++) { const int a = c.off[k], n = c.off[k + 1] - a; if (n < 3) continue;          // the call, transcribed: every triple of the plane in order
            std::vector<Vec3> ray; std::vector<Point2f> targ;
            for (int i = a; i < a + n; i++) { ray.push_back(Traits::vec3(((double)c.host_xy[2*(size_t)i] - c.K[2])/c.K[0], ((double)c.host_xy[2*(size_t)i + 1] - c.K[3])/c.K[1], c.rho_out[(size_t)i]));
                const Point2f t = { c.targ_xy[2*(size_t)i], c.targ_xy[2*(size_t)i + 1] }; targ.push_back(t); }
            double best = -1.0;
            for (int h = c.hyp_off[k]; h < c.hyp_off[k + 1]; h++) { Vec3 th; const size_t Idx[3] = { (size_t)c.triple[3*(size_t)h], (size_t)c.triple[3*(size_t)h + 1], (size_t)c.triple[3*(size_t)h + 2] };
                const double s = SolveTheta(Idx, c.Tcr, targ, ray, c.K, th);
                if (best < s) { best = s; c.sel[k] = h - c.hyp_off[k]; c.score[k] = s; for (int j = 0; j < 3; j++) c.theta[3*k + (size_t)j] = th(j); } } }
        tsorb_adapter::scatter_text_theta<Traits>(c, &F1);
        // the reference's loops on their own vectors, their own draws from the same seed
        g_lcg = seed; std::vector<Vec3> mNcr; std::vector<bool> vNGOOD; double Tcr[12]; Traits::tcr_of(Tcw, Trw, Tcr);
        for (int j0 = 0; j0 < nd; j0++) { mNcr.push_back(Traits::vec3(NAN, NAN, NAN)); vNGOOD.push_back(false); }
        if (mode == 0) {
            for (size_t i0 = 0; i0 < F1.vTextDeteCorMap.size(); i0++) { if (F1.vTextDeteCorMap[i0] >= 0) continue;
                if (F1.vKeysNewTextTrack[i0].size() < 8) continue;
                Vec3 theta; if (!theta_of(F1.vKeysNewTextTrack[i0], F2.vKeysTextTrack[i0], rho[i0], Tcr, K, max_it, true, theta)) continue;
                mNcr[i0] = theta; vNGOOD[i0] = true; }
        } else {                                                            // initializer.cc:131-150 draws for every plane first, :153-181 then scores
            std::vector<std::vector<std::vector<size_t> > > RansacIdx((size_t)nd, std::vector<std::vector<size_t> >((size_t)max_it, std::vector<size_t>(3, 0)));
            for (int i1 = 0; i1 < nd; i1++) if (TextKeys3D[(size_t)i1].size() >= 4) GetRANSACIdx(max_it, 3, (int)TextKeys3D[(size_t)i1].size(), RansacIdx[(size_t)i1]);
            for (int i2 = 0; i2 < nd; i2++) { const std::vector<Vec3> &Keys3D = TextKeys3D[(size_t)i2]; if (Keys3D.size() < 3) continue;
                std::vector<Point2f> targ; for (size_t i = 0; i < Keys3D.size(); i++) { const Point2f t = { (float)TextKeys2[(size_t)i2][i](0), (float)TextKeys2[(size_t)i2][i](1) }; targ.push_back(t); }
                double BestScore = -1.0; Vec3 BestTheta = Traits::vec3(-1.0, -1.0, -1.0);
                for (size_t i3 = 0; i3 < RansacIdx[(size_t)i2].size(); i3++) { Vec3 theta; const size_t Idx[3] = { RansacIdx[(size_t)i2][i3][0], RansacIdx[(size_t)i2][i3][1], RansacIdx[(size_t)i2][i3][2] };
                    const double score = SolveTheta(Idx, Tcr, targ, Keys3D, K, theta);
                    if (BestScore < score) { BestTheta = theta; BestScore = score; } }
                if (BestScore < 0) continue;
                mNcr[(size_t)i2] = BestTheta; vNGOOD[(size_t)i2] = true; }
        }
        if (mNcr.size() != F1.mNcr.size() || vNGOOD != F1.vNGOOD) FAIL("vNGOOD differs from the reference's loops");
        for (size_t i = 0; i < mNcr.size(); i++) if (memcmp(mNcr[i].v, F1.mNcr[i].v, 24) != 0 && !(std::isnan(mNcr[i](0)) && std::isnan(F1.mNcr[i](0)))) FAIL("mNcr differs from the reference's loops");
    } else {
        if (tsorb_create(&ctx, 1000, 1.2f, 8, 20, 7, 0) != TSORB_OK) FAIL("tsorb_create");
        rc = mode == 0 ? tsorb_adapter::initial_text_objs<Traits>(ctx, &F1, F2, &c, max_it)
                       : tsorb_adapter::initial_text_objs_init<Traits>(ctx, &F1, &F2, TextKeys1, TextKeys3D, TextKeys2, max_it, &c);
        if (rc != TSORB_OK) { fprintf(stderr, "tsorb_match_text_theta_ransac: %s\n", tsorb_last_error(ctx)); return 1; }
    }
    if ((int)F1.mNcr.size() != nd || (int)F1.vNGOOD.size() != nd || g_seeded < 1) FAIL("mNcr / vNGOOD have another length, or the generator was never seeded");
    const int32_t P = c.n_plane(), N = c.off.back(), H = c.hyp_off.back(), rc32 = rc;
    FILE *g = fopen(argv[host ? 3 : 2], "wb"); if (!g) FAIL("cannot open output");
    wr(g, &rc32, 1); wr(g, &P, 1); wr(g, &N, 1); wr(g, &H, 1); wr(g, c.det.data(), c.det.size()); wr(g, c.off.data(), c.off.size()); wr(g, c.hyp_off.data(), c.hyp_off.size());
    wr(g, c.triple.data(), c.triple.size()); wr(g, c.host_xy.data(), c.host_xy.size()); wr(g, c.targ_xy.data(), c.targ_xy.size()); wr(g, c.rho_out.data(), c.rho_out.size());
    wr(g, c.Tcr, 12); wr(g, c.K, 4); wr(g, c.sel.data(), c.sel.size()); wr(g, c.theta.data(), c.theta.size()); wr(g, c.score.data(), c.score.size());
    wr(g, &nd, 1);
    for (int i = 0; i < nd; i++) wr(g, F1.mNcr[(size_t)i].v, 3);
    for (int i = 0; i < nd; i++) { const uint8_t b = F1.vNGOOD[(size_t)i] ? 1 : 0; wr(g, &b, 1); }
    fclose(g);
    if (ctx) tsorb_destroy(ctx);
    printf(host ? "text theta from C++ (host): ok\n" : "text theta from C++: ok\n");
    return 0;
}
