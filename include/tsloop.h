/* tsloop.h -- C ABI of the loop-closure optimisers (libtsloop.so, gfx950).  SURVEY.md 8f rank 4.
 *
 *   optimizer::OptimizeSim3   /root/reference/src/optimizer.cc:626-731  (auto_sim.h, auto_siminv.h)   -> tsloop_optimize_sim3
 *   optimizer::OptimizeLoop   /root/reference/src/optimizer.cc:733-957  (numer_loop_ver2.h, ModelTool.hpp:354-432 logSim3) -> tsloop_optimize_loop
 *   Sim3Solver::iterate + optimizer::OptimizeSim3 per loop candidate  src/Sim3Solver.cc:59-253             -> tsloop_sim3_batch
 *   loopClosing::DetectLoop   src/loopClosing.cc:119-304  (tool::LevenshteinDist, src/tool.cc:264-299)       -> tsloop_detect_loop
 *
 * Same Levenberg-Marquardt semantics as the BA library (Ceres 1.x TrustRegionMinimizer + LevenbergMarquardtStrategy with Jacobi
 * scaling), fp64.  All functions return 0 on success, a negative TSLOOP_ERR_* otherwise. */
#ifndef TSLOOP_H
#define TSLOOP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TSLOOP_OK 0
#define TSLOOP_ERR_ARG (-1)
#define TSLOOP_ERR_DEVICE (-2)
#define TSLOOP_ERR_NUMERIC (-3)

typedef struct tsloop_options {
    int32_t max_it;                    /* options.max_num_iterations = 20, optimizer.cc:676 */
    int32_t pad;
    double  huber_delta;               /* HuberLoss(sqrt(10)), optimizer.cc:661 */
    double  thresh_outlier;            /* 4.0 px, optimizer.cc:629 */
    /* Ceres 1.x defaults */
    double  initial_radius, max_radius, min_radius, min_relative_decrease;
    double  function_tolerance, gradient_tolerance, parameter_tolerance, min_diagonal, max_diagonal;
} tsloop_options;

typedef struct tsloop_report {
    int32_t iters, accepted, termination;   /* termination: 0 max-iter, 1 function tol, 2 parameter tol, 3 gradient tol, 4 radius, 5 failure */
    int32_t n_inlier;                       /* return value of OptimizeSim3 */
    double  cost0, cost1;
    double  t_ms;
} tsloop_report;

/* Sim3 between two keyframes from n 3D-2D matches in both directions (optimizer::OptimizeSim3).
 * P1 / P2: vFeat1[i].posObv / vFeat2[i].posObv (the matched point in camera-1 / camera-2 coordinates), [n][3];
 * uv1 / uv2: vFeat1[i].obv2d.pt / vFeat2[i].obv2d.pt, [n][2] float;  inlier: vbInliers, [n], in/out;
 * sim: Sim12 = (qw qx qy qz | t | s), in/out (q is normalised on entry as the reference does). */
typedef struct tsloop_sim3_problem {
    int32_t n, pad;
    const double *P1, *P2;
    const float  *uv1, *uv2;
    uint8_t *inlier;
    double K[4];                            /* fx fy cx cy (K1 = K2 = K, optimizer.cc:633-634) */
    double sim[8];
} tsloop_sim3_problem;

/* Sim3 pose graph over the keyframes of the map (optimizer::OptimizeLoop).
 * pose: [n_kf][8] = (qw qx qy qz | t | s) per keyframe, the initial values of optimizer.cc:745-778 (vScwIni), in/out;
 * fixed: [n_kf], 1 = SetParameterBlockConstant (keyframes 0, 1 and the loop keyframe, :861-869);
 * one residual block per connection e: keyframes (edge_i[e], edge_j[e]) in AddResidualBlock order and the measured Sji = meas[e]
 * (q | t | s), both the normal (:788-820) and the loop (:823-858) connections.  The map update that follows the solve in the
 * reference (SetPose, rho *= s, theta *= s, :884-956) stays with the caller. */
typedef struct tsloop_graph_problem {
    int32_t n_kf, n_edge;
    double *pose;
    const uint8_t *fixed;
    const int32_t *edge_i, *edge_j;
    const double *meas;
} tsloop_graph_problem;

/* Every loop candidate's Sim3Solver RANSAC and OptimizeSim3 in one launch (loopClosing::ComputeSim3, src/loopClosing.cc:306-377;
 * Sim3Solver::iterate / ComputeSim3 / CheckInliers / Project, src/Sim3Solver.cc:59-253; docs/sim3solver_recalled.md).
 * Flat and candidate-major: candidate k's matches are rows [off[k], off[k+1]) of the per-match arrays, its hypotheses rows
 * [hyp_off[k], hyp_off[k+1]) of triple -- the three match indices (relative to the candidate) each hypothesis is formed from, in
 * the order the hypotheses run.  The caller draws them (adapter/tsloop_sim3_ransac.hpp): at most TSLOOP_RANSAC_MAX_HYP per candidate.
 *   P1 / P2 [n][3]: vFeat{Cur,Can}[i].posObv;  pred1 / pred2 [n][2]: obv2dPred (what RANSAC tests against);
 *   uv1 / uv2 [n][2] float: obv2d.pt (what the LM uses, as tsloop_sim3_problem);
 *   K1: the current keyframe's fx fy cx cy;  K2 [n_cand][4]: each candidate's own;  K: the LM's, as tsloop_sim3_problem.K;
 *   min_inliers (20, mRansacMinInliers), max_err2 (45.0, MaxError1 = MaxError2);  optimise: 1 = the LM runs on every ok candidate.
 * Per candidate: ok = the return value of iterate();  sel = the selected hypothesis (relative; -1: the candidate has none, and
 * then n_inlier_ransac = 0 and sim_ransac = 0);  n_inlier_ransac = its inlier count;  sim_ransac [8] = it as (qw qx qy qz | t | s),
 * q normalised, qw >= 0;  sim [8] / rep = the LM's result from sim_ransac and the selected mask -- not written for a candidate that
 * is not ok, nor when optimise == 0 (rep.t_ms is the whole call's time);  inlier [n]: the selected hypothesis' mask, reduced by the
 * LM's thresh_outlier test when optimise, all 0 for a candidate that is not ok.
 * hyp_count [hyp_off[n_cand]] / hyp_sim [..][8] (either may be NULL): every hypothesis' inlier count and Sim3. */
#define TSLOOP_RANSAC_MAX_HYP 64
typedef struct tsloop_sim3_batch_problem {
    int32_t n_cand, optimise;
    const int32_t *off, *hyp_off, *triple;
    const double *P1, *P2, *pred1, *pred2;
    const float  *uv1, *uv2;
    const double *K2;
    double K1[4], K[4];
    int32_t min_inliers, pad;
    double max_err2;
    uint8_t *ok;
    int32_t *sel, *n_inlier_ransac;
    double *sim_ransac, *sim;
    tsloop_report *rep;
    uint8_t *inlier;
    int32_t *hyp_count;
    double *hyp_sim;
} tsloop_sim3_batch_problem;

/* loopClosing::DetectLoop (src/loopClosing.cc:119-304): the Levenshtein scan of every text the current keyframe observes against every text object of the map,
 * the match lists, the vote through the matched objects' observing keyframes and the candidate walk, in one call (three launches, integers and one fp64 quotient).
 * Strings are bytes, flat behind offsets: query q is q_str[q_off[q] .. q_off[q+1]), map text m is m_str[m_off[m] .. m_off[m+1]), at most TSLOOP_TEXT_MAX_LEN each.
 *   pair (q, m): dist = the DP of tool::LevenshteinDist (src/tool.cc:281-296) over bytes, maxlen = max(len_q, len_m), score = (double)(maxlen - dist) / (double)maxlen.
 *     Not scored (the reference's -1): m_skip[m] (STATE == TEXTBAD, :180), m == q_self[q] (:184), and maxlen == 0 -- a stated difference: the reference divides 0 / 0.
 *   query q: ScoreMax = its largest score; no match if nothing is scored or ScoreMax < min_str_score (:203).  Scoreth = ScoreMax if ScoreMax == 1.0, else
 *     max(ScoreMax*2.0/3.0, score_thresh_min) in fp64 in that order (:207-210).  Its matches are the scored m with !(score < Scoreth) (:216), in descending score,
 *     equal scores by ascending m -- the order of a stable sort; the second stated difference: std::sort (:199) leaves equal scores in an unspecified order.
 *   votes: kf_score[k] = the (q, matched m) pairs with k in m's row of obs_kf (:255), kf_nobj[k] = the distinct matched m with k in their row (:258-261).  The rows
 *     hold only ELIGIBLE keyframes -- those the tests of :230-245 let through -- as indices into the caller's vKFs.
 *   candidates: the keyframes with kf_score > min_matched_words && kf_nobj > min_matched_words by descending kf_score, equal scores by ascending index, the first
 *     min(top_n, n_kf) of them: the walk of :277-300 (break on the score, continue on the object count, break at TopN).  The CovisibleNum test of :294-296 cannot
 *     fire for an eligible keyframe: eligibility (:232) already requires that entry of vM[0] to be 0.
 * Outputs: match_cnt [n_query]; of query q entries [0, match_cnt[q]) of row q of match_idx / match_dist / match_score ([n_query][max_match]; the rest of the row
 * is not written); kf_score / kf_nobj [n_kf]; n_cand and cand[0 .. n_cand) (cand holds top_n; the rest is not written). */
#define TSLOOP_TEXT_MAX_LEN 64          /* bytes of one recognition string */
typedef struct tsloop_detect_problem {
    int32_t n_query, n_map, n_kf, top_n;          /* top_n: TopN = 10, loopClosing.cc:273 */
    const int32_t *q_off;  const uint8_t *q_str;  /* [n_query + 1] byte offsets, the bytes of textCur.mean */
    const int32_t *q_self;                        /* [n_query] map index of the query's own object (:184), or -1 */
    const int32_t *m_off;  const uint8_t *m_str;  /* [n_map + 1], the bytes of every map text's TextMean.mean */
    const uint8_t *m_skip;                        /* [n_map] 1 = STATE == TEXTBAD (:180) */
    const int32_t *obs_off, *obs_kf;              /* [n_map + 1], [obs_off[n_map]]: the ELIGIBLE keyframes observing map text m,
                                                     as indices in [0, n_kf), strictly increasing inside a row */
    double  min_str_score, score_thresh_min;      /* 0.3 (:122);  ScoreThresh_min 0.51 / 0.35 (:30,36) */
    int32_t min_matched_words, max_match;         /* MinMatchedWords;  capacity of a query's match list */
    /* out */
    int32_t *match_cnt;                           /* [n_query] */
    int32_t *match_idx, *match_dist;              /* [n_query][max_match] */
    double  *match_score;                         /* [n_query][max_match] */
    int32_t *kf_score, *kf_nobj;                  /* [n_kf]: vMapKFScore[k].second, vKFsMathedObjs[k].size() */
    int32_t *n_cand, *cand;                       /* [1], [top_n]: vMatchKFs as keyframe indices, in the reference's order */
} tsloop_detect_problem;

void tsloop_default_options_sim3(tsloop_options *o);
void tsloop_default_options_loop(tsloop_options *o);    /* 20 iterations, no loss (huber_delta / thresh_outlier unused) */
int  tsloop_create(int device, void **ctx);          /* TSLOOP_ERR_DEVICE without a usable GPU: there is no CPU path */
void tsloop_destroy(void *ctx);
const char *tsloop_last_error(void *ctx);
int  tsloop_optimize_sim3(void *ctx, tsloop_sim3_problem *p, const tsloop_options *o, tsloop_report *r);
int  tsloop_optimize_loop(void *ctx, tsloop_graph_problem *p, const tsloop_options *o, tsloop_report *r);   /* r->n_inlier unused */
void tsloop_default_options_sim3_ransac(tsloop_sim3_batch_problem *p);    /* min_inliers = 20, max_err2 = 45.0, optimise = 1; nothing else is touched */
/* TSLOOP_OK also when candidates are not ok (a result, not an error); TSLOOP_ERR_NUMERIC when an LM solve ends with termination 5
 * (every output is complete, rep[k].termination says which); TSLOOP_ERR_ARG -- nothing launched, no output touched, tsloop_last_error
 * names the function -- for a NULL pointer where data is needed, a negative count, offsets that do not start at 0 or decrease, more
 * than TSLOOP_RANSAC_MAX_HYP hypotheses of a candidate, a triple index outside the candidate or twice in a triple, a non-finite P,
 * pred, uv or K, min_inliers < 0, a non-finite or negative max_err2, more than INT32_MAX / 3 matches in all.  n_cand == 0 returns
 * TSLOOP_OK and reads no pointer. */
int  tsloop_sim3_batch(void *ctx, tsloop_sim3_batch_problem *p, const tsloop_options *o);
void tsloop_default_options_detect(tsloop_detect_problem *p);   /* min_str_score = 0.3, score_thresh_min = 0.51, top_n = 10, max_match = 64; nothing else is touched */
/* TSLOOP_OK with n_query == 0 (no pointer is read; kf_score, kf_nobj and n_cand are zeroed where they are not NULL) and with n_map == 0 (match_cnt, kf_score,
 * kf_nobj and n_cand are zeroed): nothing is launched.  TSLOOP_ERR_ARG -- nothing launched, no output touched, tsloop_last_error names the function -- for a NULL
 * pointer where data is needed, a negative count, top_n < 1, max_match < 1, min_matched_words < 0, a non-finite threshold, offsets that do not start at 0 or
 * decrease, a string longer than TSLOOP_TEXT_MAX_LEN, q_self outside [-1, n_map), an obs_kf outside [0, n_kf) or not strictly increasing in its row.
 * A query with more matches than max_match: match_cnt, kf_score, kf_nobj, n_cand and cand are complete (the votes do not depend on the lists), that query's list
 * is not written, and the call returns TSLOOP_ERR_ARG with a message that says so (tsorb_text_extract's convention for cap): call again with the largest match_cnt. */
int  tsloop_detect_loop(void *ctx, tsloop_detect_problem *p);

#ifdef __cplusplus
}
#endif
#endif
