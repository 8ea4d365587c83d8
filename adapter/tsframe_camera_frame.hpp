// tsframe_camera_frame.hpp -- header-only replacement of the first stage of a camera frame.  The reference undistorts on the host
// (cv::undistort(im, imUn, K, dist, K), main.cpp:73), converts to grey on the host (cvtColor BGR2GRAY / RGB2GRAY, src/tracking.cc:69-73), and an
// integration then uploads that grey image twice: into the ORB context (tsorb_extract_batch) and into the pyramid context (tsframe_set_image).
// grab_frame sends the RAW frame up once: tsframe_set_raw_image undistorts it, converts it and builds the BA pyramid on the device
// (include/tsframe.h; tsframe_set_camera once per camera beforehand), and tsorb_extract_device takes the resident grey level 0 by a device-to-device
// copy (include/tsorb.h).  Both contexts must be on the same device.  C++11, no OpenCV: the image is a pointer and a row stride, or any type with
// cv::Mat's members data, step and channels() (a mock in tests/cxx/camera_frame_from_cxx.cpp).
#ifndef TSFRAME_CAMERA_FRAME_HPP
#define TSFRAME_CAMERA_FRAME_HPP
#include <stdint.h>
#include <cstddef>
#include <vector>
#include "tsframe.h"
#include "tsorb.h"

namespace tsframe_adapter {

// One raw image in; the pyramid resident in pyr_ctx, the scene keypoints (6 floats each: pt.x, pt.y, size, angle, response, octave) and their
// 32-byte descriptors out, and the ORB batch resident in orb_ctx as after tsorb_extract_batch on the undistorted grey image.
// undist_out: NULL, or [h][w][channels] for the undistorted image in raw's channel order (e.g. for the text detector's input).
// Returns the number of keypoints; < 0: the TSFRAME_ERR_* / TSORB_ERR_* of the call that refused (tsframe_last_error / tsorb_last_error name it),
// kp6 and desc are then empty.
inline int grab_frame(void *pyr_ctx, void *orb_ctx, const uint8_t *raw, int stride, int format, int n_levels,
                      std::vector<float> &kp6, std::vector<uint8_t> &desc, uint8_t *undist_out = 0) {
    kp6.clear(); desc.clear();
    int rc = tsframe_set_raw_image(pyr_ctx, raw, stride, format, n_levels, undist_out);
    if (rc != TSFRAME_OK) return rc;
    int w = 0, h = 0; const uint8_t *grey = 0;
    if ((rc = tsframe_level_size(pyr_ctx, 0, &w, &h)) != TSFRAME_OK || (rc = tsframe_level_ptr(pyr_ctx, 0, TSFRAME_IMG, &grey)) != TSFRAME_OK) return rc;
    const int nl = tsorb_get_levels(orb_ctx);
    if (nl < 1) return TSORB_ERR_ARG;
    std::vector<int32_t> per_level((size_t)nl, 0);
    if ((rc = tsorb_get_features_per_level(orb_ctx, per_level.data())) != TSORB_OK) return rc;
    int cap = 8*nl + 64;                                             // ExtractorCore::capacity(): nfeatures + 8 * nlevels + 64
    for (int l = 0; l < nl; l++) cap += per_level[(size_t)l];
    kp6.resize(6*(size_t)cap); desc.resize(32*(size_t)cap); int32_t n = 0;
    rc = tsorb_extract_device(orb_ctx, grey, 1, w, h, w, kp6.data(), desc.data(), &n, cap);
    if (rc != TSORB_OK) { kp6.clear(); desc.clear(); return rc; }
    kp6.resize(6*(size_t)n); desc.resize(32*(size_t)n);
    return n;
}

// The same over an image type with cv::Mat's members: data, step (bytes per row) and channels() (1: grey; 3: BGR, or RGB with rgb = true, the
// reference's mbRGB).  The size is the camera's (tsframe_set_camera).
template <class Img>
int grab_frame(void *pyr_ctx, void *orb_ctx, const Img &im, bool rgb, int n_levels, std::vector<float> &kp6, std::vector<uint8_t> &desc,
               uint8_t *undist_out = 0) {
    const int ch = im.channels();
    if (ch != 1 && ch != 3) { kp6.clear(); desc.clear(); return TSFRAME_ERR_ARG; }
    const int format = ch == 1 ? TSFRAME_RAW_GREY : rgb ? TSFRAME_RAW_RGB : TSFRAME_RAW_BGR;
    return grab_frame(pyr_ctx, orb_ctx, (const uint8_t *)im.data, (int)im.step, format, n_levels, kp6, desc, undist_out);
}

}  // namespace tsframe_adapter
#endif
