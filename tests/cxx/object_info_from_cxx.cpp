// TEST INFRASTRUCTURE: mapText::GetObjectInfo for a keyframe's new text objects (tsframe_text_object_info) driven from C++ through
// adapter/tsframe_text_object_info.hpp over mock types with the shape of Eigen's Vec2 / Mat31 / Mat33 and TextSLAM's TextFeature / mapText.
//
//   object_info_from_cxx <in.bin> <out.bin>
//     in.bin (tests/test_gpu_object_info.py): int32 w, h, n_levels, n_dete; double inv[n_levels]; double K[n_levels][4] (fx, fy, cx, cy); the image
//     (w x h, 8-bit); per detection: int32 good, double quad[8], per level: int32 m, m x (double u, v, featureInten).
//     1. one context with the pyramid through tsframe_set_image;
//     2. text_object_info over all detections (those that are not good have no object);
//     3. writes per good detection: double statistics[n_levels][2], vTextDete[n_levels][8], vTextDeteRay[8]; per level: int32 count, per feature
//        double featureNInten, neighbourInten[8], neighbourNInten[8], neighbour[8][2], neighbourRay[8][3], int32 number of neighbours, uint8 INITIAL, IN;
//        then vRefPixs: int32 count, per pixel double u, v, feature(0), feature(1), featureInten, featureNInten, ray(0..2), int32 level, IdxToRaw,
//        uint8 INITIAL, IN; then int32 vRefFeatureSTATE.size() and the number of true entries.
//   Prints "object info from C++: ok" and exits 0, 3 without a HIP device, anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tsframe_text_object_info.hpp"

namespace mocko {
struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat31 { double v[3]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat33 { double m[9]; double operator()(int r, int c) const { return m[3*r + c]; } double &operator()(int r, int c) { return m[3*r + c]; } };
struct TextFeature {                                            // a poisoned constructor: every field the reference sets must be set by the adapter
    double u, v; Vec2 feature; int level, IdxToRaw; bool INITIAL; Mat31 ray; double featureInten, featureNInten; bool IN;
    std::vector<Vec2> neighbour; std::vector<Mat31> neighbourRay; std::vector<double> neighbourInten, neighbourNInten;
    TextFeature() : u(-1), v(-1), level(-1), IdxToRaw(-1), INITIAL(true), featureInten(-1), featureNInten(-1), IN(false) { feature.v[0] = feature.v[1] = -1; ray.v[0] = ray.v[1] = ray.v[2] = -1; }
};
struct mapText {
    std::vector<std::vector<Vec2> > vTextDete; std::vector<Vec2> vTextDeteRay, statistics;
    std::vector<std::vector<TextFeature *> > vRefFeature; std::vector<TextFeature *> vRefPixs; std::vector<bool> vRefFeatureSTATE;
};
}  // namespace mocko
using namespace mocko;

template <class T> static bool rd(FILE *f, T *p, size_t k) { return k == 0 || fread(p, sizeof(T), k, f) == k; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    int32_t hd[4];
    if (!rd(f, hd, 4)) return 2;
    const int w = hd[0], h = hd[1], nl = hd[2], nd = hd[3];
    if (w < 2 || h < 2 || nl < 1 || nl > TSFRAME_MAX_LEVELS || nd < 0) return 2;
    std::vector<double> inv((size_t)nl), kk(4*(size_t)nl);
    std::vector<uint8_t> img((size_t)w*h);
    if (!rd(f, inv.data(), inv.size()) || !rd(f, kk.data(), kk.size()) || !rd(f, img.data(), img.size())) return 2;
    std::vector<Mat33> vK((size_t)nl);
    for (int l = 0; l < nl; l++) { memset(vK[(size_t)l].m, 0, sizeof vK[(size_t)l].m); vK[(size_t)l](0, 0) = kk[4*(size_t)l]; vK[(size_t)l](1, 1) = kk[4*(size_t)l + 1]; vK[(size_t)l](0, 2) = kk[4*(size_t)l + 2]; vK[(size_t)l](1, 2) = kk[4*(size_t)l + 3]; vK[(size_t)l](2, 2) = 1.0; }
    std::vector<bool> vNGOOD((size_t)nd);
    std::vector<std::vector<Vec2> > vTextDete((size_t)nd);
    std::vector<mapText *> objs((size_t)nd, (mapText *)0);
    size_t nfeat = 0;
    for (int i = 0; i < nd; i++) {
        int32_t good; double q[8];
        if (!rd(f, &good, 1) || !rd(f, q, 8)) return 2;
        vNGOOD[(size_t)i] = good != 0;
        for (int k = 0; k < 4; k++) { Vec2 p; p.v[0] = q[2*k]; p.v[1] = q[2*k + 1]; vTextDete[(size_t)i].push_back(p); }
        mapText *t = good ? new mapText() : (mapText *)0;       // the constructor's part: vRefFeature = vfeatureText[i]
        if (t) t->vRefFeature.resize((size_t)nl);
        for (int l = 0; l < nl; l++) {
            int32_t m; if (!rd(f, &m, 1) || m < 0) return 2;
            std::vector<double> d(3*(size_t)m); if (!rd(f, d.data(), d.size())) return 2;
            for (int k = 0; t && k < m; k++) {
                TextFeature *tf = new TextFeature();
                tf->u = d[3*(size_t)k]; tf->v = d[3*(size_t)k + 1]; tf->featureInten = d[3*(size_t)k + 2]; tf->level = l; tf->IdxToRaw = k; tf->INITIAL = false;
                t->vRefFeature[(size_t)l].push_back(tf); nfeat++;
            }
        }
        objs[(size_t)i] = t;
    }
    fclose(f);

    void *ctx = nullptr;
    if (tsframe_create(0, &ctx) != TSFRAME_OK) { printf("no HIP device\n"); return 3; }
    // a context without an image: an error, and the objects stay as they were
    if (tsframe_adapter::text_object_info(ctx, vNGOOD, vTextDete, objs, inv, vK) == TSFRAME_OK) { fprintf(stderr, "no error without an image\n"); return 1; }
    for (int i = 0; i < nd; i++) if (objs[(size_t)i] && (!objs[(size_t)i]->statistics.empty() || !objs[(size_t)i]->vRefPixs.empty())) { fprintf(stderr, "touched after an error\n"); return 1; }
    if (tsframe_set_image(ctx, img.data(), w, h, nl) != TSFRAME_OK) { fprintf(stderr, "set_image: %s\n", tsframe_last_error(ctx)); return 1; }
    const int rc = tsframe_adapter::text_object_info(ctx, vNGOOD, vTextDete, objs, inv, vK);
    if (rc != TSFRAME_OK) { fprintf(stderr, "tsframe_text_object_info (%d): %s\n", rc, tsframe_last_error(ctx)); return 1; }
    // a keyframe without a good detection: no call, no error
    { std::vector<bool> g0((size_t)nd, false);
      if (tsframe_adapter::text_object_info(ctx, g0, vTextDete, objs, inv, vK) != TSFRAME_OK) { fprintf(stderr, "no good detection\n"); return 1; } }
    tsframe_destroy(ctx);

    FILE *o = fopen(argv[2], "wb"); if (!o) { perror(argv[2]); return 2; }
    size_t npix = 0; int ngood = 0;
    for (int i = 0; i < nd; i++) {
        mapText *t = objs[(size_t)i];
        if (!t) continue;
        ngood++;
        if (t->statistics.size() != (size_t)nl || t->vTextDete.size() != (size_t)nl || t->vTextDeteRay.size() != 4) { fprintf(stderr, "shape of object %d\n", i); return 1; }
        for (int l = 0; l < nl; l++) fwrite(t->statistics[(size_t)l].v, 8, 2, o);
        for (int l = 0; l < nl; l++) { if (t->vTextDete[(size_t)l].size() != 4) return 1; for (int k = 0; k < 4; k++) fwrite(t->vTextDete[(size_t)l][(size_t)k].v, 8, 2, o); }
        for (int k = 0; k < 4; k++) fwrite(t->vTextDeteRay[(size_t)k].v, 8, 2, o);
        for (int l = 0; l < nl; l++) {
            const int32_t m = (int32_t)t->vRefFeature[(size_t)l].size();
            fwrite(&m, 4, 1, o);
            for (int k = 0; k < m; k++) {
                TextFeature *tf = t->vRefFeature[(size_t)l][(size_t)k];
                const int32_t nn = (int32_t)tf->neighbour.size();
                if (tf->neighbourRay.size() != (size_t)nn || tf->neighbourInten.size() != (size_t)nn || tf->neighbourNInten.size() != (size_t)nn || (nn != 0 && nn != 8)) { fprintf(stderr, "neighbours of %d %d %d\n", i, l, k); return 1; }
                double d[1 + 8 + 8 + 16 + 24]; memset(d, 0, sizeof d);
                d[0] = tf->featureNInten;
                for (int q = 0; q < nn; q++) {
                    d[1 + q] = tf->neighbourInten[(size_t)q]; d[9 + q] = tf->neighbourNInten[(size_t)q];
                    d[17 + 2*q] = tf->neighbour[(size_t)q].v[0]; d[18 + 2*q] = tf->neighbour[(size_t)q].v[1];
                    for (int r = 0; r < 3; r++) d[33 + 3*q + r] = tf->neighbourRay[(size_t)q].v[r];
                }
                const uint8_t b[2] = { (uint8_t)tf->INITIAL, (uint8_t)tf->IN };
                fwrite(d, 8, 57, o); fwrite(&nn, 4, 1, o); fwrite(b, 1, 2, o);
                delete tf;
            }
        }
        const int32_t m = (int32_t)t->vRefPixs.size();
        fwrite(&m, 4, 1, o);
        for (int k = 0; k < m; k++) {
            TextFeature *tf = t->vRefPixs[(size_t)k];
            const double d[9] = { tf->u, tf->v, tf->feature(0), tf->feature(1), tf->featureInten, tf->featureNInten, tf->ray(0), tf->ray(1), tf->ray(2) };
            const int32_t q[2] = { tf->level, tf->IdxToRaw }; const uint8_t b[2] = { (uint8_t)tf->INITIAL, (uint8_t)tf->IN };
            fwrite(d, 8, 9, o); fwrite(q, 4, 2, o); fwrite(b, 1, 2, o);
            delete tf;
        }
        npix += (size_t)m;
        int32_t st[2] = { (int32_t)t->vRefFeatureSTATE.size(), 0 };
        for (size_t k = 0; k < t->vRefFeatureSTATE.size(); k++) st[1] += t->vRefFeatureSTATE[k] ? 1 : 0;
        fwrite(st, 4, 2, o);
        delete t;
    }
    fclose(o);
    printf("object info from C++: ok (%d objects, %zu features, %zu pixels)\n", ngood, nfeat, npix);
    return 0;
}
