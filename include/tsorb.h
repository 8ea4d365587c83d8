/*
 * tsorb.h -- C ABI of the MI355X-native ORB front-end (the ORBextractor hot path of TextSLAM).
 *
 *   tsorb_create         <- ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)   src/ORBextractor.cc:410-471
 *   tsorb_extract_batch  <- ORBextractor::operator()(image, mask, keypoints, descriptors)                      src/ORBextractor.cc:1054-1116
 *                           = ComputePyramid (:1118-1143) + ComputeKeyPointsOctTree (:766-854: per-cell cv::FAST 20 -> 7,
 *                             DistributeOctTree :540-764, IC_Angle :77-104) + GaussianBlur 7x7 sigma 2 + computeOrbDescriptor (:108-147)
 *
 * The reference extracts one frame per call on one CPU thread; this ABI takes a batch of frames (frame::FeatExtraScene calls
 * it once per frame, frame.cc:328-331 -- the adapter simply passes n = 1, or batches the two initialisation frames).
 * Keypoints come back in the reference's order (level-major, quadtree list order inside a level) as 6 floats
 * (x, y, size, angle, response, octave) = the cv::KeyPoint fields the reference fills; descriptors as 32 bytes each.
 * All pointers are HOST pointers owned by the caller.  Return 0 = OK, negative = error; never exits.
 */
#ifndef TSORB_H
#define TSORB_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TSORB_OK          0
#define TSORB_ERR_ARG    -1
#define TSORB_ERR_DEVICE -2
#define TSORB_MAX_LEVELS  8

int tsorb_create(void **ctx, int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast, int device);
int tsorb_destroy(void *ctx);
const char *tsorb_last_error(void *ctx);

/* Getters of the reference class (ORBextractor.h:63-88): scale factors / per-level feature quota. */
int tsorb_get_levels(void *ctx);
int tsorb_get_scale_factors(void *ctx, float *sf /*[nlevels]*/, float *inv_sf /*[nlevels]*/);
int tsorb_get_features_per_level(void *ctx, int32_t *n /*[nlevels]*/);

/* imgs: n grayscale frames, each h rows of `stride` bytes (w <= stride).
 * kp [n][cap][6], desc [n][cap][32], count [n]: per frame at most cap keypoints (the reference returns <= ~nfeatures + a few). */
int tsorb_extract_batch(void *ctx, const uint8_t *imgs, int n, int w, int h, int stride,
                        float *kp, uint8_t *desc, int32_t *count, int cap);

/* Staged form for resident benchmarking: upload once, run the device pipeline any number of times, download.
 * Geometry: any w, h >= 64 and stride >= w (odd sizes, row-padded images: the pad bytes are never part of any output), with two limits that are the reference's own
 * divisions by zero, on every level l of the pyramid (w_l = cvRound(w / scale^l), h_l likewise):
 *   - w_l >= 62 and h_l >= 62: ComputeKeyPointsOctTree's grid has (int)((side - 32) / 30) cells per direction (8 levels at scale 1.2: sides from 221);
 *   - round((w_l - 32) / (h_l - 32)) >= 1: DistributeOctTree starts from that many nodes, so a search area more than twice as high as wide cannot be distributed.
 * Outside them, and for n < 1, cap < 1, a NULL pointer or stride < w: TSORB_ERR_ARG, tsorb_last_error names the reason, nothing is launched, no output of
 * tsorb_extract_batch is touched and the resident batch stays as it was. */
int tsorb_upload(void *ctx, const uint8_t *imgs, int n, int w, int h, int stride, int cap);
/* tsorb_upload / tsorb_extract_batch with the batch already on the context's device, e.g. level 0 of a resident BA pyramid
 * (tsframe_level_ptr(0, TSFRAME_IMG) of include/tsframe.h after tsframe_set_raw_image: n = 1, stride = w).  The same checks, geometry and same-geometry
 * fast path as the host forms (one body); the pixels reach the context by a device-to-device copy on its stream, which is waited for before
 * tsorb_upload_device returns, so the source may change afterwards.  The results are those of the host forms on the same bytes.
 * TSORB_ERR_ARG, with nothing touched, also for a dev_imgs that hipPointerGetAttributes does not report as device memory of the context's device, or whose
 * allocation ends before n * h rows of stride bytes (a host pointer is refused, not read). */
int tsorb_upload_device(void *ctx, const uint8_t *dev_imgs, int n, int w, int h, int stride, int cap);
int tsorb_extract_device(void *ctx, const uint8_t *dev_imgs, int n, int w, int h, int stride,
                         float *kp, uint8_t *desc, int32_t *count, int cap);
int tsorb_run(void *ctx);
int tsorb_download(void *ctx, float *kp, uint8_t *desc, int32_t *count);

/* Test hook: pyramid level `level` (with its 19-px BORDER_REFLECT_101 frame) of frame f after a run: (h_l + 38) x (w_l + 38) bytes;
 * blurred = 1 returns the 7x7 Gaussian-blurred level (no frame): h_l x w_l. */
int tsorb_debug_level(void *ctx, int frame, int level, int blurred, uint8_t *out, int32_t *w_out, int32_t *h_out);
/* Test / diagnostics hook: the shape of the FAST launch(es).  -1 (default): chosen by the batch size -- from 24 frames on, the levels whose cells fit a 40 x 40
 * tile run two waves per cell in a launch of their own, the others (and every level of a smaller batch) four waves per cell on a 72 x 72 tile; 0: every level through
 * the general instance whatever the batch size; 2: the split whatever the batch size; 1 / 3: the split with four waves / one wave per cell on the small tile (A/B runs).
 * The output does not depend on it (tests/test_gpu_orb.py).  Takes effect at the next upload. */
int tsorb_debug_fast_shape(void *ctx, int shape);
/* Test / diagnostics hook: how the pyramid is formed.  -1 (default): chosen by the batch size -- for a few frames a tile of a level is formed from a base level several
 * levels up inside one workgroup (k_pyramid_one: two launches, levels 0 .. 3 from the input image and levels 4 .. from level 3; the per-frame call of frame.cc:328-331 is
 * a chain of eight dependent launches otherwise), larger batches take a launch per level; 0: always a launch per level; 1: always the two launches; 2: every level from
 * the input image in ONE launch (when the geometry fits the kernel's buffers; a launch per level otherwise); 3: two levels per launch at any batch size (an experiment:
 * slower on a batch); 100 + s: the two launches split at level s (takes effect at the next upload); 200 / 201: a batch's orientation and blur as two launches / one (default).
 * Up to 5 frames take the few-frames plan (where it still beats the batch plan, which gained from the same session's work).  The output is the same bytes every way (tests/test_gpu_orb.py). */
int tsorb_debug_pyramid(void *ctx, int shape);
/* Test hook: the number of runs of this context in which a (frame, level) did not fit the LDS quadtree (more than 4096 candidates, 1024 nodes) and the serial pass
 * (k_octree_serial, then orientation and descriptors once more) was launched behind the first synchronisation. */
int tsorb_debug_fallbacks(void *ctx);

/* ---- Window / projection search: the step between the extractor and PoseOptim.
 *   tsorb_match_set_frame / _set_features  <- frame::AssignFeaturesToGrid + PosInGrid                       src/frame.cc:372-407
 *   tsorb_match_search                     <- frame::GetFeaturesInArea (src/frame.cc:415-468; keyframe.cc:217-256 with qlev = -1,-1)
 *                                             + tracking::DescriptorDistance (src/tracking.cc:2762-2778) + the best / second-best scan
 *                                             of tracking::SearchFrom3D / SearchFrom3DAdd / SearchFrom3DLocalTrack (:1109-1345)
 * The searched frame is frame `frame` of the resident batch (its keypoints and descriptors never leave the device) or an explicit
 * feature set (kp6 [n][6] = x,y,size,angle,response,octave as the extractor returns them; desc [n][32]).  min/max x/y are the
 * frame's mnMinX.. (frame.cc:115-125); the grid is FRAME_GRID_COLS x FRAME_GRID_ROWS = 64 x 48.
 * Per query (x, y, radius r, octave range qlev = {minLevel, maxLevel}, NULL = no level check, 32-byte descriptor):
 *   cand_idx / cand_dist [nq][max_cand]: the candidates in the reference's order with their Hamming distances (cand_cnt = how many
 *   there were, possibly > max_cand), best_idx / best_dist: the first minimum (strict <, as the reference's loop; -1 / INT_MAX if
 *   none), best_dist2: the runner-up distance.  Stateful variants (SearchForInitializ's running vMatchDist filter, the
 *   first-come claim of a feature) can stay in the caller, on the candidate lists; tsorb_match_search_claim and
 *   tsorb_match_new_points below run them on the device.  Output pointers may be NULL. */
int tsorb_match_set_frame(void *ctx, int frame, double min_x, double max_x, double min_y, double max_y);
int tsorb_match_set_features(void *ctx, const float *kp6, const uint8_t *desc, int n, double min_x, double max_x, double min_y, double max_y);
int tsorb_match_search(void *ctx, int nq, const float *qxy, const float *qr, const int32_t *qlev, const uint8_t *qdesc, int max_cand,
                       int32_t *cand_idx, int32_t *cand_dist, int32_t *cand_cnt, int32_t *best_idx, int32_t *best_dist, int32_t *best_dist2);

/* ---- All-pairs matching of loop closing: loopClosing::SearchMatch for every loop candidate of ComputeSim3 (src/loopClosing.cc:306-377, :738-925).
 * Both calls need only a context: no resident batch, and the resident batch and the match grid are left as they were.  Host pointers in, host pointers out.
 * Offset arrays start at 0 and never decrease; a set (a pair's queries or train rows, the current keyframe's features, a candidate's features) has at most
 * TSORB_BRUTE_MAX_FEAT rows: a feature index then fits the 16 low bits of the (distance << 16 | index) key the device reduces, whose distance field (0 .. 256, and
 * 0x7fff for "none") stays below 2^15, so the key never leaves a positive int32.
 *
 *   tsorb_match_brute_text   <- loopClosing::FeatureMatch_brute(Descrip1, Descrip2, USETHRESH = true) (:1491-1519) for n_pair (query set, train set) pairs: per
 *     query row the nearest train row of ITS pair by 256-bit Hamming distance (cv::BFMatcher("BruteForce-Hamming")::match as docs/bfmatcher_recalled.md states it:
 *     one match per query, the first index on a tie), train_idx relative to the pair, dist its distance, good = dist < max(2 min_dist, 30.0) in doubles with
 *     min_dist the minimum over the pair's queries.  The reference's good_matches are the good rows in query order.  A pair without queries writes nothing; a pair
 *     with an empty train set gives train_idx -1, dist INT32_MAX, good 0 (the reference skips such pairs: loopClosing.cc:799).
 *   tsorb_match_brute_scene  <- loopClosing::SearchMatch_Other (:823-925) for n_cand candidates against the current keyframe's n1 features, the candidates independent
 *     of each other.  has3d = the reference's Cond1 evaluated by the caller (scene feature: vMatches2D3D >= 0; text feature: vTextDeteCorMap[vTextObjInfo] >= 0).
 *     Cond2: candidate k's boxes are rows [qoff[k], qoff[k+1]) of quad_cur (painted into the current keyframe's label image by SearchMatch_Text for this candidate)
 *     and of quad_can (into the candidate's); a feature is out when one of its image's boxes covers the pixel ((int)roundf(x), (int)roundf(y)) in the sense of
 *     cv::fillPoly on a w x h image (corners truncated like cv::Point(double, double), boundary included); a rounded pixel outside the image is not covered (the
 *     reference reads out of bounds there).  Then the reference's scan, exactly: i1 in index order, the first minimum and the runner-up distance over the eligible i2
 *     with !(vMatchDist[i2] <= dist), accepted when best <= th_low && best < (double)second*ratio (second = INT_MAX when there is none), a later i1 taking an i2 from
 *     an earlier one.  match12 [n_cand][n1] = vMatchIdx12 (-1 = none), n_match [n_cand] = nMatches = the entries >= 0 of the row.  th_low 50 and ratio 0.9 are the
 *     reference's values.
 * n_pair == 0 / n_cand == 0: TSORB_OK, no pointer is read.  n1 == 0: n_match = 0, nothing is launched.  TSORB_ERR_ARG (tsorb_last_error names the function, nothing is
 * launched, no output is touched) for: a NULL context or a NULL pointer where data is needed, a negative count, an offset array that does not start at 0 or
 * decreases, w or h outside [1, 8192], a coordinate that is not finite, a quad corner that is not finite or beyond 2^30, th_low outside [0, 256], a ratio that is
 * not finite or negative, a set above TSORB_BRUTE_MAX_FEAT. */
#define TSORB_BRUTE_MAX_FEAT 65536
int tsorb_match_brute_text(void *ctx, int n_pair,
                           const int32_t *off1 /*[n_pair+1]*/, const uint8_t *desc1 /*[off1[n_pair]][32]*/,
                           const int32_t *off2 /*[n_pair+1]*/, const uint8_t *desc2 /*[off2[n_pair]][32]*/,
                           int32_t *train_idx /*[off1[n_pair]]*/, int32_t *dist /*[off1[n_pair]]*/, uint8_t *good /*[off1[n_pair]]*/);
int tsorb_match_brute_scene(void *ctx, int w, int h,
                            int n1, const float *xy1 /*[n1][2]*/, const uint8_t *desc1 /*[n1][32]*/, const uint8_t *has3d1 /*[n1]*/,
                            int n_cand, const int32_t *off2 /*[n_cand+1]*/, const float *xy2, const uint8_t *desc2, const uint8_t *has3d2,
                            const int32_t *qoff /*[n_cand+1]*/, const double *quad_cur /*[qoff[n_cand]][4][2]*/, const double *quad_can /*same*/,
                            int th_low, double ratio, int32_t *match12 /*[n_cand][n1]*/, int32_t *n_match /*[n_cand]*/);

/* ---- Window searches in many feature sets: loop fusion.  loopClosing::SearchAndFuse_Scene (src/loopClosing.cc:1168-1288) projects every loop map point into the current
 * keyframe and into each of its connected keyframes and scans keyframe::GetFeaturesInArea(u, v, 15) (src/keyframe.cc:217-256) with DescriptorDistance, a host loop of
 * K keyframes x P points; loopClosing::MatchMore (:1398-1489) does the same per loop candidate.  Here every (set, query) pair of such a step goes to ONE call: a grid launch
 * (a workgroup per set) and a search launch (a wave per query).
 *   Set s = rows [foff[s], foff[s+1]) of kp6 / desc with bounds[s] = min_x, max_x, min_y, max_y (the keyframe's mnMinX ..).  Query q searches set qset[q] at qxy[q] with
 *   radius qr[q], octave range qlev[q] (NULL = no level check, keyframe::GetFeaturesInArea) and descriptor row qdi[q] of qdesc (NULL = row q; then n_qdesc == nq): K
 *   keyframes searched with the same P descriptors send them once.
 * Query q gets exactly what tsorb_match_set_features(kp6 + 6 foff[s], desc + 32 foff[s], foff[s+1] - foff[s], bounds[s]) followed by a one-query tsorb_match_search returns:
 * the candidates in the reference's order (window cells column by column, features in index order inside a cell), the Hamming distances, the first minimum under strict <,
 * the runner-up distance, -1 / INT32_MAX when there is none; indices relative to the set.  Output pointers may be NULL; max_cand = 0: no candidate lists.
 * Needs only a context: the resident batch and the single-set grid of tsorb_match_set_* are left as they were.  n_set == 0 or nq == 0: TSORB_OK, no pointer is read.  A set
 * without features is legal (cand_cnt 0, -1, INT32_MAX, INT32_MAX).  TSORB_ERR_ARG (tsorb_last_error names the function, nothing is launched, no output is touched) for: a
 * NULL context or a NULL pointer where data is needed, a negative count, n_set > TSORB_SETS_MAX, a foff that does not start at 0 or decreases, a set above
 * TSORB_BRUTE_MAX_FEAT rows, bounds with max <= min or not finite, a qset outside [0, n_set), a qdi outside [0, n_qdesc), qdi == NULL with n_qdesc != nq, a query
 * coordinate or radius that is not finite, max_cand < 0. */
#define TSORB_SETS_MAX 1024
int tsorb_match_search_sets(void *ctx,
        int n_set, const int32_t *foff /*[n_set+1]*/, const float *kp6 /*[foff[n_set]][6]*/, const uint8_t *desc /*[foff[n_set]][32]*/,
        const double *bounds /*[n_set][4] = min_x, max_x, min_y, max_y*/,
        int n_qdesc, const uint8_t *qdesc /*[n_qdesc][32]*/,
        int nq, const int32_t *qset /*[nq]*/, const int32_t *qdi /*[nq] row of qdesc, NULL = the query's own index (then n_qdesc == nq)*/,
        const float *qxy /*[nq][2]*/, const float *qr /*[nq]*/, const int32_t *qlev /*[nq][2], NULL = no level check*/,
        int max_cand, int32_t *cand_idx, int32_t *cand_dist, int32_t *cand_cnt, int32_t *best_idx, int32_t *best_dist, int32_t *best_dist2);

/* ---- The outlier gate between the window search and PoseOptim: tracking::CheckMatch (src/tracking.cc:1499-1579), called by TrackWithMotMod / TrackWithOutMod as soon as
 * more than 20 matches survive, = cv::solvePnPRansac(vP3d, vP2d, K, 0, rvec, tvec, false, 100, ReproError, 0.98, inliers, SOLVEPNP_EPNP) as docs/pnpransac_recalled.md states
 * it: up to n_hyp five-point EPnP hypotheses, an inlier count of each over all n matches, the loop with RANSACUpdateNumIters' early stop.  The refit on the inliers that
 * follows changes rvec / tvec only, which CheckMatch does not read: it is not built.
 *   Pw [n][3]: the matches' world points as floats (OpenCV converts vP3d to CV_32F), uv [n][2]: their keypoints, K = fx, fy, cx, cy (EPnP runs on pixel coordinates).
 *   subset [n_hyp][5]: the hypotheses' matches.  The library has no generator: the caller draws them (adapter/tsorb_pnp_check.hpp restates cv::RNG's draws).
 *   ALL n_hyp hypotheses are evaluated and reported: hyp_count [n_hyp] = each one's inlier count (err <= (float)(reproj_err^2), no test on the depth's sign), hyp_pose
 *   [n_hyp][12] = its R | t, 3 x 4 row-major.  result = { ok, n_inlier, sel, n_run }: the reference's loop over the counts keeps hypothesis sel (-1: none; a count must
 *   exceed max(maxGood, 4), the first of equal counts stays) with n_inlier = maxGood inliers, would have run n_run hypotheses, and succeeds (ok) iff maxGood > 0.
 *   inlier [n] = the kept hypothesis' mask, all 0 when not ok; pose [12] = its R | t (zeros when not ok).  pose, hyp_count, hyp_pose may be NULL.
 * A degenerate subset (five points whose scatter has an eigenvalue ratio below 1e-12: coplanar, collinear, coincident) is a result, not an error: its pose is NaN and
 * its count is what the comparisons give (a NaN compares false: 0).  Needs only a context: the resident batch and the match grid are left as they were.
 * TSORB_ERR_ARG (tsorb_last_error names the function, nothing is launched, no output is touched) for: a NULL context or a NULL pointer where data is needed, n < 5,
 * n > TSORB_PNP_MAX_POINTS, n_hyp outside [1, TSORB_PNP_MAX_HYP], a subset index outside [0, n) or twice in a subset, a point, pixel or K that is not finite,
 * reproj_err not finite or <= 0, confidence outside [0, 1]. */
#define TSORB_PNP_MAX_HYP 128
#define TSORB_PNP_MAX_POINTS 65536
int tsorb_match_pnp_ransac(void *ctx, int n, const float *Pw /*[n][3]*/, const float *uv /*[n][2]*/, const double K[4] /*fx fy cx cy*/,
                           int n_hyp, const int32_t *subset /*[n_hyp][5], the caller draws them*/, double reproj_err, double confidence,
                           uint8_t *inlier /*[n]*/, int32_t *result /*[4]: ok, n_inlier, sel, n_run*/, double *pose /*[12] R|t row-major, may be NULL*/,
                           int32_t *hyp_count /*[n_hyp] or NULL*/, double *hyp_pose /*[n_hyp][12] or NULL*/);

/* ---- The two-view initializer's RANSAC: initializer::FindHomography + FindFundamental (src/initializer.cc:185-284, called at :95-96 on every frame until a pair
 * initialises) with ComputeH21 / ComputeF21 (:287-364) and CheckHomography / CheckFundamental (:366-529), as docs/twoview_recalled.md states them: n_hyp eight-point
 * homography fits and n_hyp eight-point fundamental-matrix fits on the SAME subsets, each model scored over all n matches, the two keep loops.
 *   xy1, xy2 [n][2]: the matched keypoints mvKeys1[mvMatches12[i].first].pt and mvKeys2[mvMatches12[i].second].pt.
 *   norm1, norm2 = meanX, meanY, sX, sY of initializer::Normalize (:819-865) over ALL keypoints of frame 1 / frame 2: an order-dependent float loop that the caller runs
 *   (adapter/tsorb_two_view.hpp: two_view_normalize).  The library forms the normalised points (x - mean) * s with the reference's two float roundings and
 *   T = [[sX, 0, -meanX sX], [0, sY, -meanY sY], [0, 0, 1]] in floats as the reference does.
 *   subset [n_hyp][8]: the hypotheses' matches (mvSets).  The library has no generator: the caller draws them (libc rand() through DUtils::Random in the reference).
 *   The fit: A from the reference's float products; from A on in fp64 -- the unit right singular vector of A's smallest singular value (one-sided Jacobi), its
 *   largest-magnitude component positive (the first on ties); F: the 3 x 3's smallest singular value set to 0; H21i = T2^-1 Hn T1, F21i = T2^T Fn T1, each rounded to
 *   float ONCE; H12i = the fp64 adjugate-over-determinant inverse of the float H21i, rounded to float (zeros when the determinant is 0).
 *   The scoring is the reference's float arithmetic to the bit: every product and sum rounded to float as written, 1.0/(float expression) a double division rounded to
 *   float, the score the SEQUENTIAL float sum over the matches in index order (first term then second).
 *   ALL 2 n_hyp hypotheses are evaluated: hyp_score [2][n_hyp] (H first), hyp_model [2][n_hyp][9] (row-major 3 x 3) when not NULL.  The keep loops start from 0.0 and
 *   keep on strictly greater (the first of equal scores stays, a NaN is never kept): sel = { kept H hypothesis, kept F hypothesis }, -1 = none; score = { SH, SF };
 *   H21, F21 the kept models; inlier_h, inlier_f [n] their masks.  sel = -1 leaves that model's mask all 0, its matrix all 0 and its score 0.
 * A degenerate subset (second smallest eigenvalue of AtA at most 1e-12 times the largest: coincident or collinear points) is a result, not an error: its model is NaN
 * and its score is what the arithmetic then gives, NaN.  Needs only a context: the resident batch, its pyramid and the match grid are left as they were.
 * TSORB_ERR_ARG (tsorb_last_error names the function, nothing is launched, no output is touched) for: a NULL context or a NULL required pointer (everything but
 * hyp_score and hyp_model), n < 8, n > TSORB_TWOVIEW_MAX_POINTS, n_hyp outside [1, TSORB_TWOVIEW_MAX_HYP], a subset index outside [0, n) or twice in a subset, a
 * coordinate or norm entry that is not finite, norm[2] or norm[3] <= 0, sigma not finite or <= 0. */
#define TSORB_TWOVIEW_MAX_HYP 256
#define TSORB_TWOVIEW_MAX_POINTS 65536
int tsorb_match_two_view_ransac(void *ctx, int n,
        const float *xy1 /*[n][2] matched keypoints of frame 1*/, const float *xy2 /*[n][2] of frame 2*/,
        const float norm1[4] /*meanX, meanY, sX, sY of Normalize(mvKeys1)*/, const float norm2[4] /*of Normalize(mvKeys2)*/,
        int n_hyp, const int32_t *subset /*[n_hyp][8], the caller draws them*/, float sigma,
        uint8_t *inlier_h /*[n]*/, uint8_t *inlier_f /*[n]*/, float *H21 /*[9]*/, float *F21 /*[9]*/,
        float *score /*[2]: SH, SF*/, int32_t *sel /*[2]: kept H hypothesis, kept F hypothesis, -1 = none*/,
        float *hyp_score /*[2][n_hyp] or NULL*/, float *hyp_model /*[2][n_hyp][9] or NULL; H rows first*/);

/* ---- The two-view initializer's reconstruction: initializer::ReconstructH (src/initializer.cc:636-802) or ReconstructF (:531-634, DecomposeE :979-999) with CheckRT
 * (:868-977) and Triangulate (:804-817), as docs/twoview_reconstruct_recalled.md states them: the model's 8 (H, Faugeras) or 4 (F) motion hypotheses, every inlier
 * match triangulated and checked under every hypothesis, the keep logic.  The RH decision between the two models (:99-102) is the caller's.
 *   xy1, xy2 [n][2] as above; inlier [n]: vbMatchesInliers of the chosen model (non-zero = inlier); model 0: M21 is H21 (ReconstructH), 1: M21 is F21 (ReconstructF);
 *   K = fx, fy, cx, cy, the floats of mK; min_parallax and min_triangulated are 1.0 and 50 at the reference's call site.
 *   The hypotheses: fp64 from the float M21 and K (A = K^-1 H K or E = K^T F K, the 3 x 3 SVD by a one-sided Jacobi iteration, the Faugeras / DecomposeE formulas),
 *   each R and t rounded to float ONCE.  Their order is fixed by a sign rule, not by an SVD routine's signs (docs): H: v1 and v3 with their largest-magnitude component
 *   positive; F: t likewise, R1 the rotation with the larger trace, (R1, t), (R2, t), (R1, -t), (R2, -t).
 *   CheckRT, given the float R, t, K: P2, O2 and R p + t with double accumulation and one float rounding per entry; Triangulate's 4 x 4 from the reference's float
 *   products, its null vector in fp64, the point rounded to float ONCE; everything after the float point is the reference's arithmetic to the bit.
 *   result [6] = ok, sel (the kept hypothesis; -1 unless ok), N (inlier count), best nGood, second best nGood (H) or nsimilar (F), exit bits: 1 = H only, d1/d2 or
 *   d2/d3 below 1.00001 (nothing is evaluated, every hyp_* output is zero), 2 = not enough good points, 4 = no clear winner, 8 = parallax.
 *   R21 [9], t21 [3], p3d [n][3], triangulated [n]: the kept hypothesis' pose, the points of its counted matches (vP3D; zeros elsewhere) and vbTriangulated, per MATCH
 *   (the reference indexes them by mvMatches12[i].first: the adapter scatters).  ok = 0 leaves all four zero.
 *   Of every hypothesis, when not NULL: hyp_good [8] = nGood, hyp_cos [8] = the cosine CheckRT picks (sorted[min(50, nGood - 1)]; 0 when nGood = 0), hyp_parallax [8]
 *   in degrees, hyp_pose [8][12] = R | t row-major 3 x 4, hyp_p3d [8][n][3] = every evaluated match's float point, hyp_state [8][n] = the exit the match took:
 *   0 not an inlier, 1 non-finite point (or a NaN cosine: the point is exactly zero), 2 depth in camera 1, 3 depth in camera 2, 4 error in image 1, 5 error in image 2,
 *   6 good (counted) but low parallax, 7 good and triangulated.  F fills hypotheses 0 .. 3 and zeroes 4 .. 7.
 * Needs only a context: the resident batch, its pyramid and the match grid are left as they were.
 * TSORB_ERR_ARG (tsorb_last_error names the function, nothing is launched, no output is touched) for: a NULL context or a NULL required pointer (everything but the
 * hyp_* outputs), n < 1, n > TSORB_TWOVIEW_MAX_POINTS, model outside {0, 1}, a coordinate, M21 entry or K entry that is not finite, fx or fy <= 0, sigma or
 * min_parallax not finite or negative, min_triangulated negative. */
#define TSORB_TWOVIEW_REC_HYP 8        /* 8 hypotheses from H, 4 from F; the arrays below are sized for 8 */
int tsorb_match_two_view_reconstruct(void *ctx, int n,
        const float *xy1 /*[n][2]*/, const float *xy2 /*[n][2]*/, const uint8_t *inlier /*[n]: vbMatchesInliers of the chosen model, non-zero = inlier*/,
        int model /*0: ReconstructH from a homography, 1: ReconstructF from a fundamental matrix*/, const float *M21 /*[9] row-major*/,
        const float K[4] /*fx fy cx cy: mK's floats*/, float sigma, float min_parallax /*1.0*/, int min_triangulated /*50*/,
        int32_t *result /*[6]: ok, sel (-1 = none), N = inlier count, best nGood, second best nGood (H) / nsimilar (F), exit bits*/,
        float *R21 /*[9]*/, float *t21 /*[3]*/, float *p3d /*[n][3]*/, uint8_t *triangulated /*[n]*/,
        int32_t *hyp_good /*[8] or NULL*/, float *hyp_cos /*[8] or NULL: the cosine CheckRT picks*/, float *hyp_parallax /*[8] or NULL, degrees*/,
        float *hyp_pose /*[8][12] R|t row-major or NULL*/, uint8_t *hyp_state /*[8][n] or NULL*/, float *hyp_p3d /*[8][n][3] or NULL*/);

/* ---- The planes of new text detections: tracking::InitialTextObjs -> GetTextTheta -> SolveTheta (src/tracking.cc:1631-1734, 1870-1917) and the two-view
 * initializer's InitialTextObjs -> CalculateTextTheta (src/initializer.cc:111-183, 1004-1061), as docs/texttheta_recalled.md states them: for every plane (a text
 * detection's features) the triangulation of every feature, then every caller-drawn index triple's closed-form theta and its score over all the plane's features,
 * and the reference's keep loop.  All planes of a keyframe in ONE call.
 *   off [n_plane+1]: plane p owns features off[p] .. off[p+1]-1 (off[0] = 0, not decreasing); N = off[n_plane].
 *   host_xy, targ_xy [N][2]: the feature in the host keyframe (level-0 pixels) and in the target frame, the floats of the cv::Point2f.
 *   rho [N] or NULL.  NULL (tracking): every feature is triangulated between [I | 0] and Tcr as cv::triangulatePoints does on PixToCam's float points -- the 4 x 4 in
 *   double, its null vector in fp64 rounded to float as a 4-vector, divided by its last entry in float -- and rho = 1.0/(double)z.  Given (the initializer, rho from
 *   IniP3D): used as it is, p3d is zero.
 *   Tcr [12]: rows of [R | t], host -> target (Tcw * Trw.inverse()); K = fx, fy, cx, cy, the doubles of mK.
 *   hyp_off [n_plane+1]: plane p owns hypotheses hyp_off[p] .. hyp_off[p+1]-1; H = hyp_off[n_plane].  triple [H][3]: feature indices WITHIN the plane, in the order
 *   drawn (tool::GetRANSACIdx; adapter/tsorb_text_theta.hpp draws them).  Indices may repeat: such a triple gives a NaN theta and is never kept.
 *   sel [n_plane]: the kept hypothesis within the plane (`BestScore < score` from -1.0 in hypothesis order: the first of the largest scores, a NaN score never), -1:
 *   none -- also for a plane of fewer than 3 features or without hypotheses; theta [n_plane][3], score [n_plane]: the kept hypothesis' NEGATED theta (what SolveTheta
 *   returns) and its score, zeros with sel = -1.
 *   When not NULL: p3d [N][3] the triangulated float points, rho_out [N] the rho that was used, hyp_score [H] and hyp_theta [H][3] of every hypothesis (zeros for a
 *   plane of fewer than 3 features).
 * Needs only a context: the resident batch, its pyramid and the match grid are left as they were.  One copy each way, at most three launches; n_plane = 0 launches
 * nothing.  TSORB_ERR_ARG (tsorb_last_error names the function and the plane, nothing is launched, no output is touched) for: a NULL context, n_plane < 0, a NULL
 * required pointer (off, hyp_off, Tcr, K, sel, theta, score; host_xy and targ_xy when N > 0; triple when H > 0), off or hyp_off not starting at 0 or decreasing, a
 * plane of more than TSORB_THETA_MAX_FEAT features, more than TSORB_THETA_MAX_HYP hypotheses in a plane, a triple index outside [0, the plane's feature count). */
#define TSORB_THETA_MAX_FEAT 1024      /* features per plane (cv::ORB::create() keeps 500 per detection) */
#define TSORB_THETA_MAX_HYP 65536      /* hypotheses per plane (the reference draws 200) */
int tsorb_match_text_theta_ransac(void *ctx, int n_plane,
        const int32_t *off /*[n_plane+1] feature ranges*/,
        const float *host_xy /*[N][2] level-0 pixels in the host keyframe (Hostfeat / F1->vKeys[].pt)*/,
        const float *targ_xy /*[N][2] pixels in the target frame (Targfeat / F2->vKeys[].pt)*/,
        const double *rho /*[N] inverse depths, or NULL: triangulate on the device (tracking's path)*/,
        const double *Tcr /*[12] rows of [R | t], host -> target*/, const double *K /*fx fy cx cy*/,
        const int32_t *hyp_off /*[n_plane+1]*/, const int32_t *triple /*[hyp_off[n_plane]][3] indices within the plane, in the order drawn*/,
        int32_t *sel /*[n_plane] kept hypothesis within the plane, -1: none*/, double *theta /*[n_plane][3]*/, double *score /*[n_plane]*/,
        float *p3d /*[N][3] or NULL: the triangulated points (rho == NULL)*/, double *rho_out /*[N] or NULL: the rho that was used*/,
        double *hyp_score /*[H] or NULL*/, double *hyp_theta /*[H][3] or NULL*/);

/* ---- The stateful window searches: tracking::SearchForTriangular (src/tracking.cc:1347-1411, the first thing TrackNewKeyframe does) and tracking::SearchForInitializ
 * (:1045-1109, every frame until the map initialises), and behind the first GetForTriangular + CheckTriangular (:1413-1497), as docs/newpoints_recalled.md states them.
 * Both calls search the context's current grid (tsorb_match_set_frame / tsorb_match_set_features) and leave it, the resident batch and its pyramid as they were.
 *
 *   tsorb_match_search_claim: the reference's loop over the queries IN QUERY ORDER.  A query's candidates are tsorb_match_search's (GetFeaturesInArea's order: window
 *     cells column by column, index order inside a cell; the qlev filter as there).  A candidate i2 is skipped when elig2[i2] == 0 (elig2 [n2] or NULL = all eligible: the
 *     reference's `F2.vMatches2D3D[i2] < 0`) and when vMatchDist[i2] <= dist (vMatchDist starts at INT_MAX).  Over the rest: the first minimum under strict < in
 *     CANDIDATE order and the runner-up distance (INT_MAX when there is none).  Accepted when best <= th_low and, with use_ratio, (double)best < (double)second*ratio.
 *     On acceptance the previous owner of that i2 loses it (match12 = -1), then match12[q] = i2, vMatchIdx21[i2] = q, vMatchDist[i2] = best.
 *     match12 [nq] = vMatchIdx12 at the end, match_dist [nq] (or NULL) = the accepted distance or -1, n_match = the entries >= 0.
 *     The caller keeps the reference's per-feature conditions (Fea.octave > 0, vMatches2D3D[i1] >= 0, vTextObjInfo[i1] >= 0) by leaving those features out of the
 *     queries and maps query numbers back itself.  SearchForTriangular: use_ratio 0, th_low 50, qr = 80*1.2f, qlev = { octave, octave }; SearchForInitializ: use_ratio 1,
 *     ratio 0.9, qr = Win.  However many candidates a query has, it gets the reference's answer (no list is cut).
 *   tsorb_match_new_points: the same search, then for every query with match12 >= 0 GetForTriangular's point and CheckTriangular's verdict; the match never visits the
 *     host.  q_px [nq][2] = F1->vKeys[i1].pt (equal to qxy in the reference; kept separate), the other pixel is the matched feature's of the grid; Trw, Tcw [12] = the
 *     top three rows of F1->mTcw and F2.mTcw, K = fx, fy, cx, cy of F2.mK, th_reproj 9.  PixToCam in double rounded to float per coordinate; cv::triangulatePoints' 4 x 4
 *     in double, its null vector in fp64 rounded to float as a 4-vector, divided by its last entry as a float reciprocal and a float product per entry; CheckTriangular
 *     as written: the finiteness tests, R p + t left to right, (fx X)/Z + cx, u1 < 0 || v1 < 0, the squared error formed in double, rounded to float and compared with
 *     (float)th_reproj.  There is no depth test and a NaN error passes both comparisons, as in the reference.
 *     p3d [nq][3], good [nq]: per query (zeros where match12 < 0); n_good = the good ones.  The reference's vNewpts / vMatchNewpts are the good rows in query order.
 * nq == 0: TSORB_OK, n_match = 0 (n_good = 0), nothing is launched.  TSORB_ERR_ARG (tsorb_last_error names the function, nothing is launched, no output is touched) for:
 * a NULL context, no grid set, a NULL required pointer (everything but qlev, elig2 and match_dist), nq < 0, a coordinate or radius that is not finite, a negative radius,
 * th_low outside [0, 256], with use_ratio a ratio that is not finite or negative, a searched set above TSORB_BRUTE_MAX_FEAT features. */
int tsorb_match_search_claim(void *ctx, int nq, const float *qxy /*[nq][2]*/, const float *qr /*[nq]*/, const int32_t *qlev /*[nq][2] or NULL*/,
                             const uint8_t *qdesc /*[nq][32]*/, const uint8_t *elig2 /*[n2] or NULL = all*/, int th_low, int use_ratio, double ratio,
                             int32_t *match12 /*[nq]*/, int32_t *match_dist /*[nq] or NULL*/, int32_t *n_match);
int tsorb_match_new_points(void *ctx, int nq, const float *qxy /*[nq][2]*/, const float *qr /*[nq]*/, const int32_t *qlev /*[nq][2] or NULL*/,
                           const uint8_t *qdesc /*[nq][32]*/, const uint8_t *elig2 /*[n2] or NULL = all*/, int th_low, int use_ratio, double ratio,
                           const float *q_px /*[nq][2]*/, const double *Trw /*[12]*/, const double *Tcw /*[12]*/, const double *K /*fx fy cx cy*/, int th_reproj /*9*/,
                           int32_t *match12 /*[nq]*/, int32_t *n_match, float *p3d /*[nq][3]*/, uint8_t *good /*[nq]*/, int32_t *n_good);

/* ---- Text features of a frame.
 * frame::FeatExtracText (src/frame.cc:334-355): for each of n_dete detection quads (level-0 pixels, double x, y; truncated like cv::Point)
 * cv::ORB::create()->detect on the frame masked to the quad (tool::GetMask) and ->compute on the frame itself, OpenCV 3.3 defaults;
 * docs/cvorb_recalled.md is the arithmetic.  frame = index in the resident batch (after tsorb_extract_batch / tsorb_upload + tsorb_run).
 * nfeatures: 500 is the drop-in value.  kp [n_dete][cap][6] = x, y, size, angle, response (Harris), octave; desc [n_dete][cap][32];
 * count [n_dete].  A detection with more than cap keypoints: TSORB_ERR_ARG with count[] complete and nothing written for that detection.
 * Only the first count[d] rows of a detection's arrays are written.  The resident batch (scene keypoints, descriptors, pyramid, match grid) is
 * left as it was.  TSORB_ERR_ARG also for: a NULL pointer with n_dete > 0, frame outside the batch or no batch resident, nfeatures < 1, cap < 1,
 * a quad coordinate that is not finite (or beyond 2^30), level 0 larger than 640 x 480.  n_dete == 0 launches nothing.
 * Two deliberate differences from OpenCV, both in docs/cvorb_recalled.md:
 *   ties   OpenCV's retainBest(n) keeps the points at or above the response of whatever std::nth_element left at position n - 1, which depends on
 *          the standard library; here a cut keeps EVERY point whose response is >= the n-th largest response (the superset of all those outcomes);
 *   order  OpenCV's order inside a level is what nth_element and partition left; here it is level-major and, inside a level, raster order of the
 *          level coordinates (y, then x).
 * These are the RAW text features: the -3-px boundary test of frame.cc:244 (tool::BoundFeatDele_T) and frame::FeatFusion are tsorb_fuse_frame below, which runs
 * this extraction itself. */
int tsorb_text_extract(void *ctx, int frame, int n_dete, const double *quad /*[n_dete][4][2]*/, int nfeatures, int cap,
                       float *kp, uint8_t *desc, int32_t *count);

/* ---- The frame's searched set: steps 3 - 4 of frame::FeatExtract, frame::FeatFusion and frame::AssignFeaturesToGrid (src/frame.cc:229-325, :372-394) in one call on
 * frame `frame` of the resident batch.  Everything the tracker searches indexes this fused set (vKeys / mDescr, vMatches2D3D, vTextObjInfo); tsorb_match_set_frame
 * alone grids the scene features only.
 *   raw text features  exactly tsorb_text_extract(ctx, frame, n_dete, quad, nfeatures, cap_text, ..): the same launches, writing device scratch; raw_count [n_dete].
 *   filter             tool::BoundFeatDele_T (src/tool.cc:456-508): raw keypoint (x, y) of detection d is kept iff CheckPtsIn(shrunk_d) && CheckPtsIn(bb_d), with
 *                      shrunk_d = (x0 - win, y0 - win), (x1 + win, y1 - win), (x2 + win, y2 + win), (x3 - win, y3 + win) formed in double and truncated like
 *                      cv::Point(double, double), bb_d = (minx, miny), (maxx, miny), (maxx, maxy), (minx, maxy) of bbox[d] = vTextDeteMin x, y, vTextDeteMax x, y truncated
 *                      the same way, and CheckPtsIn = cv::pointPolygonTest(int contour, Point2f, true) > 0 as docs/pointpolygon_recalled.md states it.  win = -3 is
 *                      the reference's WinText.  (BoundFeatDele_S never runs in the reference, FLAG_NOSCENEMASK is hard-coded: the scene rows are not filtered.)
 *   fusion             rows [0, n_scene) = the resident frame's keypoints and descriptors as tsorb_download returns them, then the kept rows of detection 0, 1, .. in
 *                      raw order.  kp [cap][6], desc [cap][32]; obj [cap] = vTextObjInfo (-1 for a scene row, d for a text row); src [cap] (or NULL) = the row itself
 *                      for a scene row, the row's index among its detection's raw keypoints for a text row (IdxNewText); text_off [n_dete + 1]: detection d's rows
 *                      are text_off[d] .. text_off[d + 1] - 1 (vKeysTextIdx[d]); n_out = { n_scene, n }.  Only the first n rows are written.
 *   grid               on success the fused set is the context's searched set, with the bounds as in tsorb_match_set_features: tsorb_match_search, _search_claim and
 *                      _new_points afterwards answer with fused indices, byte for byte what they answer after tsorb_match_set_features(kp, desc, n, bounds).
 * The resident batch (scene outputs, pyramid, what tsorb_download returns) is left as it was; a later tsorb_text_extract gives the same bytes.
 * n_dete == 0: the fused set is the scene set, no pointer of the detection arrays is read.
 * Capacity: a detection with more than cap_text raw keypoints, or n > cap: TSORB_ERR_ARG with raw_count and n_out written, nothing else written, and the searched set
 * what it was.  raw_count is complete in both cases, and so is n_out when only cap was too small; a detection that does not fit cap_text has no rows to test, so n then
 * counts the others only (cap_text = the largest raw_count and cap = n_scene + the sum of raw_count always suffice for a second call).
 * TSORB_ERR_ARG (tsorb_last_error names the function, nothing is launched, no output is touched) also for: a NULL context, no batch resident or frame outside it, a NULL
 * required pointer (src and raw_count may be NULL; quad and bbox with n_dete == 0), n_dete < 0, nfeatures < 1, cap_text < 1, cap < 1, a quad or bbox value or win that
 * is not finite or lies beyond 2^30, bounds with max <= min or not finite, level 0 larger than 640 x 480 (tsorb_text_extract's cap).
 * One pinned block up, the 13 launches of the text extraction, k_fuse_keep / k_fuse_offsets / k_fuse_gather (csrc/tsfuse.h), one pinned block down, one wait, then the
 * grid's launches. */
int tsorb_fuse_frame(void *ctx, int frame, int n_dete,
                     const double *quad /*[n_dete][4][2] vTextDete, level-0 pixels*/, const double *bbox /*[n_dete][4] = vTextDeteMin x, y, vTextDeteMax x, y*/,
                     double win /*-3: WinText of frame.cc:237*/, int nfeatures /*500*/, int cap_text /*raw rows per detection*/, int cap /*fused rows*/,
                     double min_x, double max_x, double min_y, double max_y /*mnMinX .. of the grid*/,
                     float *kp /*[cap][6]*/, uint8_t *desc /*[cap][32]*/, int32_t *obj /*[cap] vTextObjInfo*/, int32_t *src /*[cap] or NULL*/,
                     int32_t *text_off /*[n_dete + 1]*/, int32_t *raw_count /*[n_dete] or NULL*/, int32_t *n_out /*[2] = n_scene, n*/);

#ifdef __cplusplus
}
#endif
#endif
