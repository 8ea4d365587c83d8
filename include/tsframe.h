/* tsframe.h -- C ABI of the BA-pyramid / reference-feature front-end (libtsframe.so, gfx950).  SURVEY.md 8f rank 3.
 *
 * Replaces, on the device and bit-exactly (integer image arithmetic; fp64 sampling without FMA contraction):
 *   frame::GetPyrMat                    /root/reference/src/frame.cc:178-204     -> tsframe_set_image
 *   tool::GetPyramidPts (text, scene)   /root/reference/src/tool.cc:564-710,862-980 -> tsframe_pyramid_pts
 *   frame::TextFeaProc (its loop)       src/frame.cc:359-370, with the scene call src/tracking.cc:420 (also :333-334, :494) -> tsframe_pyramid_pts_batch
 *   tool::CalNormvec / GetNeighbour     /root/reference/src/tool.cc:1342-1364,1540-1566 (INTERVAL8) -> tsframe_neighbours
 *   tool::GetBoxAllPixs                 /root/reference/src/tool.cc:1264-1337     -> tsframe_box_pixels
 *   tracking::TextJudgeSingle (xn)      /root/reference/src/tracking.cc:1991-2131 -> tsframe_text_judge
 *   tracking::TrackNewTextFeat          /root/reference/src/tracking.cc:1752-1785 -> tsframe_klt_track
 *   mapText::GetObjectInfo              src/mapText.cc:64-107 (tool::CalTextinfo src/tool.cc:1178-1262, CalNormvec :1342-1355,
 *                                       GetBoxAllPixs :1264-1337; callers src/tracking.cc:932-957 and InitialLandmarker) -> tsframe_text_object_info
 *   cv::undistort + cvtColor            main.cpp:73, src/tracking.cc:69-73 (docs/undistort_recalled.md) -> tsframe_set_camera, tsframe_set_raw_image
 * The pyramid stays resident in HBM: tsframe_level_ptr hands the device pointers to the BA library, so the four levels of a
 * keyframe need no host round trip between GetPyrMat and the photometric residuals.
 * All functions return 0 on success, a negative TSFRAME_ERR_* otherwise; tsframe_last_error gives the text. */
#ifndef TSFRAME_H
#define TSFRAME_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TSFRAME_OK 0
#define TSFRAME_ERR_ARG (-1)
#define TSFRAME_ERR_DEVICE (-2)
#define TSFRAME_ERR_STATE (-3)
#define TSFRAME_MAX_LEVELS 8

enum { TSFRAME_IMG = 0, TSFRAME_GRAD = 1, TSFRAME_GRADX = 2, TSFRAME_GRADY = 3 };

int tsframe_create(int device, void **ctx);
void tsframe_destroy(void *ctx);
const char *tsframe_last_error(void *ctx);

/* frame::GetPyrMat: level 0 = img (w x h, 8-bit), level l = cv::pyrDown(level l-1); per level cv::Sobel x / y (CV_8U) and their
 * addWeighted(.5, .5) blend.  The image is copied through a pinned staging buffer; everything else happens on the device. */
int tsframe_set_image(void *ctx, const uint8_t *img, int w, int h, int n_levels);

/* The camera-frame entry: cv::undistort(im, imUn, K, dist, K_new) (main.cpp:73), cvtColor BGR2GRAY / RGB2GRAY
 * (src/tracking.cc:69-73) and frame::GetPyrMat from ONE upload of the raw frame.  The arithmetic is docs/undistort_recalled.md (OpenCV 3.3's
 * non-IPP path as recalled; everything after the fixed-point map is integer), restated in tests/camera_frame_ref.py.
 * tsframe_set_camera, once per camera: builds cv::initUndistortRectifyMap's CV_16SC2 map for a w x h image on the device, strip by strip as
 * cv::undistort does, and keeps it until the next call (which may change the size).  K = fx fy cx cy, dist = k1 k2 p1 p2 k3, K_new = the new
 * camera matrix (NULL: K, the reference's call).
 * tsframe_set_raw_image, per frame: raw = h rows of stride bytes, 8-bit BGR, RGB (3 bytes per pixel) or grey (1), row-padded or not; w, h are the
 * camera's.  The frame goes to the device in one copy through the pinned staging; one kernel remaps it (INTER_LINEAR, BORDER_CONSTANT 0, per
 * channel), converts the rounded channels to grey and stores level 0; then the chain of tsframe_set_image runs unchanged.  Afterwards every other
 * call behaves as after tsframe_set_image(grey, w, h, n_levels) with grey = the undistorted grey image (bit for bit), and
 * tsframe_level_ptr(0, TSFRAME_IMG) is what tsorb_extract_device (include/tsorb.h) takes.  undist_out: NULL, or [h][w][channels] for the undistorted
 * image before the grey conversion, in raw's channel order (one copy back).
 * tsframe_get_undist_map, test hook: the resident map, xy [h][w][2] = (short)(iu >> 5), (short)(iv >> 5) and frac [h][w] = (iv & 31) * 32 + (iu & 31).
 * TSFRAME_ERR_ARG: a NULL pointer (K_new and undist_out may be NULL), w or h < 2 or above 8192, a non-finite K / dist / K_new, fx or fy == 0 in K or
 * K_new, a format other than the three, stride < w * channels, n_levels outside [1, 8].  TSFRAME_ERR_STATE: a frame or a map request before a camera
 * is set.  On any of them nothing is launched, the resident planes and map stay as they were, no output is touched, and tsframe_last_error names
 * the function.  Not covered: k4 - k6, thin-prism and tilt coefficients, a rectification rotation. */
#define TSFRAME_RAW_BGR 0
#define TSFRAME_RAW_RGB 1
#define TSFRAME_RAW_GREY 2
int tsframe_set_camera(void *ctx, int w, int h, const double K[4] /*fx fy cx cy*/, const double dist[5] /*k1 k2 p1 p2 k3*/,
                       const double K_new[4] /*NULL: K*/);
int tsframe_set_raw_image(void *ctx, const uint8_t *raw, int stride, int format, int n_levels,
                          uint8_t *undist_out /*NULL, or [h][w][channels]: the undistorted image before the grey conversion*/);
int tsframe_get_undist_map(void *ctx, int16_t *xy /*[h][w][2]*/, uint16_t *frac /*[h][w]*/);

int tsframe_level_size(void *ctx, int level, int *w, int *h);
/* device pointer of a resident plane (which = TSFRAME_IMG / GRAD / GRADX / GRADY); valid until the next tsframe_set_image */
int tsframe_level_ptr(void *ctx, int level, int which, const uint8_t **dev);
int tsframe_get_level(void *ctx, int level, int which, uint8_t *out);

/* tool::GetPyramidPts.  mode 0: text features, grid over the detection box box = {PMin.x, PMin.y, PMax.x, PMax.y} (level-0 pixels);
 * mode 1: scene features, grid over the image (box ignored).  xy = n raw features (float x, y at level 0), inv_scale[n_levels].
 * Outputs are level-major, level l in [level_off[l], level_off[l+1]); capacity of every output array: n * n_levels.
 * u, v: level coordinates; idx: IdxToRaw; inten: bilinear intensity on the level image; in: the bilinear sample was inside.
 * This is tsframe_pyramid_pts_batch for one set: the same kernel in one launch, with this call's own argument checks.  TSFRAME_ERR_ARG: a NULL
 * pointer (xy only with n > 0; box only with mode 0), n < 0, a mode other than 0 or 1, a grid that is degenerate at some level (cw < 1 or
 * ch < 1: an empty box) or exceeds 2^31 - 1 cells, n * n_levels above INT32_MAX.  Coordinates are not checked for finiteness or magnitude.
 * TSFRAME_ERR_STATE: no image set.  On any error no output array is touched; n == 0 gives a zero level_off. */
int tsframe_pyramid_pts(void *ctx, int mode, const float *xy, int n, const double *box, const double *inv_scale,
                        int32_t *level_off, double *u, double *v, int32_t *idx, double *inten, uint8_t *in);

/* tool::GetPyramidPts for all feature sets of a frame (every text detection of frame::TextFeaProc, and the scene observations) in ONE kernel
 * launch.  Set i: mode[i] (0 text / 1 scene), its n_i = xy_off[i+1] - xy_off[i] raw features xy[xy_off[i] ..], box[i][4] (read for mode-0 sets only;
 * box may be NULL without one); inv_scale[n_levels].  With L = the context's n_levels, set i owns the elements [xy_off[i]*L, xy_off[i+1]*L) of u, v,
 * idx, inten and in, and row i of level_off[n_set][L + 1]; inside that range the contents and their order, the level_off row (relative to the set's
 * base) and idx (relative to the set's first feature) are exactly what tsframe_pyramid_pts writes for that set alone (it is this call with one
 * set), so a loop over the single call can be swapped for this one.  The sets are independent of each other.  The inputs go to the device as one block through the pinned
 * staging, one kernel runs (one workgroup per set and level, whatever n_set and n_levels are), the results come back in one copy.
 * n_set == 0 returns TSFRAME_OK without reading any pointer; with n_set > 0 and no feature at all nothing is launched and level_off is zeroed.
 * TSFRAME_ERR_ARG (tsframe_last_error names this function and, where it applies, the set): a NULL pointer where data is needed, n_set < 0, a mode
 * other than 0 or 1, xy_off[0] != 0 or a decreasing xy_off, more than INT32_MAX / n_levels features, a set whose grid is degenerate at some level
 * (cw < 1 or ch < 1: an empty box) or exceeds 2^31 - 1 cells, as in the single call, and a coordinate of xy, of a mode-0 box or of inv_scale that is not finite or above
 * 2^20 in magnitude.  That last bound keeps the cell index inside an int on the device and in the CPU restatement alike; the single call does not
 * check it.  TSFRAME_ERR_STATE: no image set.  On any error nothing is launched and no output array is touched. */
int tsframe_pyramid_pts_batch(void *ctx, int n_set, const int32_t *mode /*[n_set], 0 text / 1 scene*/,
                              const int32_t *xy_off /*[n_set + 1]*/, const float *xy /*[xy_off[n_set]][2]*/,
                              const double *box /*[n_set][4], read for mode-0 sets only*/, const double *inv_scale /*[n_levels]*/,
                              int32_t *level_off /*[n_set][n_levels + 1]*/, double *u, double *v, int32_t *idx, double *inten, uint8_t *in);

/* tool::CalNormvec -> GetNeighbour(INTERVAL8) on the resident level image: for n features (uv, level coordinates) the 8 neighbour
 * intensities, raw and (I - mu) / sigma; in[j] = inside flag of the last tap (what the reference leaves in feat->IN).
 * sigma == 0: TSFRAME_ERR_ARG (the reference's CalNormvec returns false). */
int tsframe_neighbours(void *ctx, int level, const double *uv, int n, double mu, double sigma,
                       double *inten8, double *ninten8, uint8_t *in);

/* tool::GetBoxAllPixs (called for level 0 by mapText's constructor, mapText.cc:103): every pixel of the level image inside the filled
 * detection quad (4 corners x, y in level pixels; cv::Point truncation + cv::fillPoly scan conversion, boundary included), in row-major
 * order of the clamped bounding box; entry i is the TextFeature with IdxToRaw = i: u, v = pixel, inten = I(v, u), ninten = (I - mu) / sigma
 * (the ray ((u - cx) / fx, (v - cy) / fy, 1) is left to the caller).  *n_out = number of pixels; cap = capacity of the four output
 * arrays, cap == 0 only counts (outputs may be NULL); n_out > cap: TSFRAME_ERR_ARG with *n_out set. */
int tsframe_box_pixels(void *ctx, int level, const double *quad, double mu, double sigma, int cap, int32_t *n_out,
                       int32_t *u, int32_t *v, double *inten, double *ninten);

/* Reasons of tsframe_text_judge, in the order the reference tests them. */
#define TSFRAME_JUDGE_PASS 0
#define TSFRAME_JUDGE_ORIENT 1   /* tool::CheckOrientation: |cos| < cos_min */
#define TSFRAME_JUDGE_DEPTH 2    /* a projected box corner has depth < 0 */
#define TSFRAME_JUDGE_BOX 3      /* a projected box corner is within out_margin of the image border (<=, >=) */
#define TSFRAME_JUDGE_ZNCC 4     /* tool::CheckZNCC failed: zncc < zncc_min, a constant vector, or fewer than 2 reference pixels */

/* tracking::TextJudgeSingle (/root/reference/src/tracking.cc:1991-2131) for n planes on the resident level image of this context
 * (the current frame), one launch, one workgroup per plane.
 * theta[n][3] = RefKF->mNcr[GetNidx()]; Tcr[n][12] = row-major 3x4 of F.mTcw * RefKF->mTcw.inverse() (computed by the caller);
 * box_ray[n][4][2] = vTextDeteRay.  Reference pixels (vRefPixs) in CSR: plane i owns [pix_off[i], pix_off[i+1]), pix_off[0] == 0;
 * pix_uv[][2] = int16 level-0 pixel (u, v) of the reference keyframe, pix_inten[] = featureInten.  The rays are rebuilt on the device as
 * ((u - cx) / fx, (v - cy) / fy, 1) with K_ref = {fx, fy, cx, cy} (the level-0 K the reference built them with); K = vK_scale[level] of
 * this frame.  cos_min: the reference passes 0 (its int parameter truncates the callers' 0.5), so 0 is the drop-in value; out_margin >= 0;
 * zncc_min <= -2 skips the ZNCC test.  dete_xy[n_dete][2] = vTextDeteCenter (level 0); with dete_bits non-NULL, bit j of plane i's
 * (n_dete + 31) / 32 words is set when the plane passed and detection j lies in its projected quad (cv::fillPoly on a label image of
 * the level-0 size, whatever that size is: up to 640 x 480 the filled mask is built, above it every rounded centre is tested against the same fill
 * without one; a centre outside that image is not associated).
 * Out, per plane: pass (1 / 0), reason (TSFRAME_JUDGE_*), cos, zncc (NaN when not computed or fewer than 2 pixels, -100 for a constant
 * vector, as the reference), box_uv[8] = the four projected corners (always all four).  n == 0 launches nothing.  The resident planes
 * are read in place and left unchanged. */
int tsframe_text_judge(void *ctx, int level, int n, const double *theta, const double *Tcr, const double *box_ray,
                       const int32_t *pix_off, const int16_t *pix_uv, const uint8_t *pix_inten,
                       const double K_ref[4], const double K[4], double cos_min, int out_margin, double zncc_min,
                       int n_dete, const double *dete_xy,
                       uint8_t *pass, int32_t *reason, double *cos, double *zncc, double *box_uv, uint32_t *dete_bits);

/* tracking::TrackNewTextFeat -> cv::calcOpticalFlowPyrLK (defaults: win 21, max_level 3, 30 iterations, eps 0.01, min_eig 1e-4) for
 * all n points of all detections in ONE launch, between the resident pyramids of two contexts on the same device. */
int tsframe_klt_track(void *prev_ctx, void *cur_ctx, int n, const float *prev_xy /*[n][2]*/,
                      int win, int max_level, int max_iter, double eps, double min_eig,
                      float *next_xy /*[n][2]*/, uint8_t *status /*[n]*/);
/* prev_ctx holds the image the points were seen in (the last frame or keyframe), cur_ctx the current frame; both stay as they are: the level
 * images are read in place, the Scharr derivatives are computed on the fly.  The arithmetic is docs/klt_recalled.md: the window sums are
 * exact integers rounded once to fp32, everything after them is fp32 in a fixed order, so a point's result does not depend on the other
 * points of the call.  Levels: L + 1 with L <= max_level; a level whose width or height is <= win is dropped with all coarser ones, and both
 * contexts must hold the levels that remain.  status[i] = 1: tracked; 0: the point or its track left the image by more than the window, the
 * patch is flat (min_eig), or the input is not finite (then next_xy = prev_xy).  OpenCV's err is not computed.
 * TSFRAME_ERR_ARG: a NULL pointer with n > 0, contexts on different devices, level-0 sizes that differ or are not larger than win, win even
 * or outside [3, 31], max_level outside [0, 7], max_iter outside [1, 100], eps < 0, too few resident levels.  TSFRAME_ERR_STATE: a context
 * without an image.  n == 0 launches nothing.  The points and the results travel through cur_ctx's pinned staging block and stream: the
 * previous frame's context must stay alive (and keep its image) until the call returns. */

/* mapText::GetObjectInfo (src/mapText.cc:64-107) for the n_obj new text objects of a keyframe on the resident pyramid of this context
 * (the reference keyframe), ONE launch, one workgroup per (object, level).  L = the context's n_levels.
 * In: quad = vTextDete (level-0 corners); the corners of level l are quad[k]*inv_scale[l] (one fp64 product, mapText.cc:78-81).  The features
 * (vRefFeature) are laid out as tsframe_pyramid_pts_batch writes them: object i owns the elements [feat_off[i]*L, feat_off[i+1]*L) of u, v, inten,
 * ninten, in (and eight times that of inten8 / ninten8), level l of it is [level_off[i][l], level_off[i][l+1]) behind that base; what lies past
 * level_off[i][L] in a slice is neither read nor written.
 * Per (object, level): tool::CalTextinfo (src/tool.cc:1178-1262) -- corner truncation (cv::Point), the clamped bounding box and cv::fillPoly as in
 * tsframe_box_pixels; musigma[i][l] = {mu, sigma} from the integer histogram of the masked pixels (mu is exact; sigma is the sample deviation, n - 1).
 * ok[i][l] = 1 with at least 2 pixels and sigma != 0; fewer than 2 pixels give mu = sigma = 0, a constant region keeps its mu with sigma = 0.
 * tool::CalNormvec (src/tool.cc:1342-1355) on the level's features: inten8 / ninten8 / in are what tsframe_neighbours gives with that mu, sigma, bit for
 * bit, and ninten = (inten - mu) / sigma (featureNInten).  With ok = 0 (CalNormvec returns false) the raw inten8 and in are still written, ninten and
 * ninten8 are 0.0.
 * Level 0 additionally, tool::GetBoxAllPixs (src/tool.cc:1264-1337) on the same mask: object i's pixels are [pix_off[i], pix_off[i+1]) of pix_u, pix_v,
 * pix_inten, pix_ninten, exactly what tsframe_box_pixels(level 0) writes for that quad with mu, sigma of level 0 (pix_ninten = 0.0 with ok = 0).
 * pix_off is always complete.  pix_cap = capacity of the four pixel arrays; pix_cap == 0 only counts (they may be NULL); a total above pix_cap:
 * TSFRAME_ERR_ARG with pix_off complete, the pixel arrays untouched and every other output written.  The sum of the clamped level-0 box areas bounds
 * the total, so one call suffices.
 * n_obj == 0 returns TSFRAME_OK without reading any pointer.  TSFRAME_ERR_ARG (tsframe_last_error names this function and, where it applies, the
 * object), checked before anything is launched or any output touched: a NULL pointer where data is needed, n_obj < 0, pix_cap < 0, feat_off[0] != 0
 * or a decreasing feat_off, a level_off row that does not start at 0, decreases or ends above (feat_off[i+1] - feat_off[i])*L, a corner, inv_scale
 * or scaled corner that is not finite or >= 1e9 in magnitude, a non-finite u / v, an image wider than 307200 pixels.  TSFRAME_ERR_STATE: no image
 * set.  The inputs go up as one block through the pinned staging, the results come back through it; the resident planes are left unchanged. */
int tsframe_text_object_info(void *ctx, int n_obj,
    const double *quad        /*[n_obj][4][2] vTextDete: level-0 corners*/,
    const double *inv_scale   /*[L], L = the context's n_levels*/,
    const int32_t *feat_off   /*[n_obj + 1]*/, const int32_t *level_off /*[n_obj][L + 1]*/,
    const double *u, const double *v, const double *inten,   /* vRefFeature, laid out as tsframe_pyramid_pts_batch writes it */
    int pix_cap,
    double *musigma /*[n_obj][L][2]*/, uint8_t *ok /*[n_obj][L]*/,
    double *ninten  /* featureNInten, layout of inten */, double *inten8, double *ninten8 /* [..][8], same feature index */, uint8_t *in,
    int32_t *pix_off /*[n_obj + 1]*/, int32_t *pix_u, int32_t *pix_v, double *pix_inten, double *pix_ninten);

#ifdef __cplusplus
}
#endif
#endif
