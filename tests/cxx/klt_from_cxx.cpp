// TEST INFRASTRUCTURE: tracking::TrackNewTextFeat's KLT step (tsframe_klt_track) driven from C++ through adapter/tsframe_klt.hpp over a mock
// point type with the shape of cv::Point2f.
//
//   klt_from_cxx <in.bin> <out.bin>
//     in.bin (tests/test_gpu_klt.py): int32 w, h, n_levels, n_dete; the tracked image and the current image (w x h, 8-bit); per detection:
//     int32 m, then m x (float x, y).
//     1. two contexts (tracked frame, current frame) with their pyramids through tsframe_set_image;
//     2. Trackedfeat as vector<vector<Point2f>>, one track_new_text_feat call with OpenCV's defaults;
//     3. writes per detection: int32 m, m x (float x, y), m x uint8 status to out.bin.
//   Prints "klt from C++: ok" and exits 0, 3 without a HIP device, anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tsframe_klt.hpp"

namespace mockk {
struct Point2f { float x, y; Point2f() : x(0.f), y(0.f) {} Point2f(float x_, float y_) : x(x_), y(y_) {} };
}  // namespace mockk
using mockk::Point2f;

template <class T> static bool rd(FILE *f, T *p, size_t k) { return k == 0 || fread(p, sizeof(T), k, f) == k; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"); if (!f) { perror(argv[1]); return 2; }
    int32_t hd[4];
    if (!rd(f, hd, 4)) return 2;
    const int w = hd[0], h = hd[1], nl = hd[2], nd = hd[3];
    std::vector<uint8_t> imgA((size_t)w*h), imgB((size_t)w*h);
    if (!rd(f, imgA.data(), imgA.size()) || !rd(f, imgB.data(), imgB.size())) return 2;
    std::vector<std::vector<Point2f> > Trackedfeat((size_t)nd), Curfeat;
    size_t tot = 0;
    for (int i = 0; i < nd; i++) {
        int32_t m; if (!rd(f, &m, 1) || m < 0) return 2;
        std::vector<float> xy(2*(size_t)m);
        if (!rd(f, xy.data(), xy.size())) return 2;
        for (int j = 0; j < m; j++) Trackedfeat[(size_t)i].push_back(Point2f(xy[2*(size_t)j], xy[2*(size_t)j + 1]));
        tot += (size_t)m;
    }
    fclose(f);

    void *prev = nullptr, *cur = nullptr;
    if (tsframe_create(0, &prev) != TSFRAME_OK) { printf("no HIP device\n"); return 3; }
    if (tsframe_create(0, &cur) != TSFRAME_OK) { tsframe_destroy(prev); printf("no HIP device\n"); return 3; }
    if (tsframe_set_image(prev, imgA.data(), w, h, nl) != TSFRAME_OK) { fprintf(stderr, "set_image: %s\n", tsframe_last_error(prev)); return 1; }
    if (tsframe_set_image(cur, imgB.data(), w, h, nl) != TSFRAME_OK) { fprintf(stderr, "set_image: %s\n", tsframe_last_error(cur)); return 1; }
    std::vector<std::vector<uint8_t> > status;
    const int rc = tsframe_adapter::track_new_text_feat(prev, cur, Trackedfeat, Curfeat, &status);
    if (rc != TSFRAME_OK) { fprintf(stderr, "tsframe_klt_track (%d): %s\n", rc, tsframe_last_error(cur)); return 1; }
    if (Curfeat.size() != Trackedfeat.size() || status.size() != Trackedfeat.size()) { fprintf(stderr, "outer shape\n"); return 1; }
    for (size_t i = 0; i < Trackedfeat.size(); i++)
        if (Curfeat[i].size() != Trackedfeat[i].size() || status[i].size() != Trackedfeat[i].size()) { fprintf(stderr, "inner shape of %zu\n", i); return 1; }
    // the overload without status, and a frame without any new detection: no launch, no error
    std::vector<std::vector<Point2f> > again, none_in, none_out(3);
    if (tsframe_adapter::track_new_text_feat(prev, cur, Trackedfeat, again) != TSFRAME_OK) return 1;
    for (size_t i = 0; i < Trackedfeat.size(); i++)
        for (size_t j = 0; j < Trackedfeat[i].size(); j++)
            if (memcmp(&again[i][j].x, &Curfeat[i][j].x, 4) != 0 || memcmp(&again[i][j].y, &Curfeat[i][j].y, 4) != 0) {   // bits: a non-finite input comes back as it went in
                fprintf(stderr, "second call differs\n"); return 1;
            }
    if (tsframe_adapter::track_new_text_feat(prev, cur, none_in, none_out) != TSFRAME_OK || !none_out.empty()) return 1;
    tsframe_destroy(cur); tsframe_destroy(prev);

    FILE *o = fopen(argv[2], "wb"); if (!o) { perror(argv[2]); return 2; }
    for (size_t i = 0; i < Curfeat.size(); i++) {
        const int32_t m = (int32_t)Curfeat[i].size();
        fwrite(&m, 4, 1, o);
        for (size_t j = 0; j < Curfeat[i].size(); j++) { fwrite(&Curfeat[i][j].x, 4, 1, o); fwrite(&Curfeat[i][j].y, 4, 1, o); }
        if (m) fwrite(status[i].data(), 1, (size_t)m, o);
    }
    fclose(o);
    printf("klt from C++: ok (%d detections, %zu points)\n", nd, tot);
    return 0;
}
