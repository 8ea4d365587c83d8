// camera_frame_from_cxx.cpp -- adapter/tsframe_camera_frame.hpp driven from C++ over a mock image type (cv::Mat's data / step / channels()):
// one raw frame in, the pyramid resident, keypoints and descriptors out.  tests/test_gpu_camera_frame.py compiles it with g++, writes the frame and
// the camera, runs it and compares every output byte with the Python mirror's.
//   in : int32 w, h, stride, channels, rgb, n_levels, has_K_new; double K[4], dist[5], K_new[4]; h * stride raw bytes
//   out: int32 n; float kp[n][6]; uint8 desc[n][32]; uint8 undistorted[h][w][channels]; per level int32 w_l, h_l and the four planes
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tsframe_camera_frame.hpp"

namespace mock {
struct Mat {                                                       // what grab_frame reads of a cv::Mat
    std::vector<uint8_t> buf; uint8_t *data; size_t step; int rows, cols, ch;
    int channels() const { return ch; }
};
}

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "camera frame from C++: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
    REQUIRE(argc == 3);
    FILE *f = fopen(argv[1], "rb"); REQUIRE(f);
    int32_t hd[7]; double K[4], dist[5], Kn[4];
    REQUIRE(fread(hd, sizeof(int32_t), 7, f) == 7 && fread(K, 8, 4, f) == 4 && fread(dist, 8, 5, f) == 5 && fread(Kn, 8, 4, f) == 4);
    const int w = hd[0], h = hd[1], stride = hd[2], ch = hd[3], rgb = hd[4], n_levels = hd[5], has_kn = hd[6];
    REQUIRE(w > 0 && h > 0 && stride >= w*ch && (ch == 1 || ch == 3));
    mock::Mat im; im.buf.resize((size_t)h*stride); im.data = im.buf.data(); im.step = (size_t)stride; im.rows = h; im.cols = w; im.ch = ch;
    REQUIRE(fread(im.data, 1, im.buf.size(), f) == im.buf.size());
    fclose(f);

    void *pyr = 0, *orb = 0;
    REQUIRE(tsframe_create(0, &pyr) == TSFRAME_OK);
    REQUIRE(tsorb_create(&orb, 1000, 1.2f, 8, 20, 7, 0) == TSORB_OK);
    std::vector<float> kp; std::vector<uint8_t> desc, und((size_t)w*h*ch);
    // a frame before its camera is refused and leaves the outputs empty
    REQUIRE(tsframe_adapter::grab_frame(pyr, orb, im, rgb != 0, n_levels, kp, desc) == TSFRAME_ERR_STATE && kp.empty() && desc.empty());
    REQUIRE(tsframe_set_camera(pyr, w, h, K, dist, has_kn ? Kn : 0) == TSFRAME_OK);
    const int n = tsframe_adapter::grab_frame(pyr, orb, im, rgb != 0, n_levels, kp, desc, und.data());
    if (n < 0) fprintf(stderr, "%s | %s\n", tsframe_last_error(pyr), tsorb_last_error(orb));
    REQUIRE(n >= 0 && kp.size() == 6*(size_t)n && desc.size() == 32*(size_t)n);

    FILE *o = fopen(argv[2], "wb"); REQUIRE(o);
    const int32_t n32 = n;
    fwrite(&n32, 4, 1, o); fwrite(kp.data(), 4, kp.size(), o); fwrite(desc.data(), 1, desc.size(), o); fwrite(und.data(), 1, und.size(), o);
    for (int l = 0; l < n_levels; l++) {
        int lw = 0, lh = 0; REQUIRE(tsframe_level_size(pyr, l, &lw, &lh) == TSFRAME_OK);
        const int32_t sz[2] = { lw, lh }; fwrite(sz, 4, 2, o);
        std::vector<uint8_t> plane((size_t)lw*lh);
        for (int k = 0; k < 4; k++) { REQUIRE(tsframe_get_level(pyr, l, k, plane.data()) == TSFRAME_OK); fwrite(plane.data(), 1, plane.size(), o); }
    }
    fclose(o);
    tsorb_destroy(orb); tsframe_destroy(pyr);
    printf("camera frame from C++: ok (%d keypoints)\n", n);
    return 0;
}
