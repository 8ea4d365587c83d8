/*
 * TEST INFRASTRUCTURE -- NOT PRODUCT CODE.
 *
 * CPU oracle for the TextSLAM bundle-adjustment hot path: a plain-C, fp64, single-threaded
 * restatement of the reference algorithm (cost functors + the Ceres-1.x Levenberg-Marquardt
 * behaviour the reference relies on).  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load this library; the product (textslam_amd/) never does.
 *
 * PARITY PINNED FOR THE COST FUNCTORS, UNPINNED FOR THE REST.
 * Pinned: the residual models.  The reference's twelve cost functors (include/auto_*.h, nume_*.h, numer_loop_ver2.h with
 * ModelTool.hpp's TextProj and logSim3) compile unchanged against the stand-in headers of oracle/ref_shims/; where the reference
 * tree is present the Makefile builds them into oracle/_ref/libtsref.so, and tests/test_ref_functors.py holds the residuals of
 * tsba_oracle_eval (and of the loop-closure oracle) and the scene / Sim3 Jacobians to their values, recorded in
 * tests/golden/ref_functors.npz (measured deviations: RECALLED.md).
 * Unpinned: everything the reference leaves to un-vendored Ceres / Eigen / OpenCV, none of which exists in the build container --
 * the Levenberg-Marquardt loop, the loss functions, the plus-Jacobian and numeric differentiation, cv::fillPoly behind mu / sigma,
 * problem construction and the outlier passes.  Those behaviours are recalled from the libraries' published sources (see
 * SURVEY.md 8c, RECALLED.md) and cited inline; the reference binary as a whole still cannot be built here.
 */
#ifndef TSBA_ORACLE_H
#define TSBA_ORACLE_H
#include "../include/tsba.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Same contract as tsba_eval (include/tsba.h).  options.text_jacobian selects analytic (0) or the
 * reference's Ceres CENTRAL numeric differentiation (1) for text blocks. */
int tsba_oracle_eval(const tsba_problem *p, const tsba_options *o, int level,
                     double *resid, double *jac, double *musigma, int64_t *ns, int64_t *nt);

/* tsba_oracle_eval in numeric mode (options.text_jacobian == 1, jac != NULL; else TSBA_ERR_ARG) that also records, per tap of
 * every text block, tap_code[nt][8]: TSBA_ORACLE_TAP_OUT if the unperturbed tap lies outside the image under the in/out rule,
 * TSBA_ORACLE_TAP_CELL / _INOUT if any +-delta evaluation of the central differences moved it to another pixel cell
 * (floor(u), floor(v)) / across the in/out rule.  A tap with either of the last two bits "straddles": its numeric derivative
 * differences across a kink of the bilinear interpolation, where the analytic (one-cell) derivative is not its limit. */
#define TSBA_ORACLE_TAP_CELL  1
#define TSBA_ORACLE_TAP_INOUT 2
#define TSBA_ORACLE_TAP_OUT   4
int tsba_oracle_eval_taps(const tsba_problem *p, const tsba_options *o, int level,
                          double *resid, double *jac, double *musigma, int64_t *ns, int64_t *nt, uint8_t *tap_code);

/* The outlier pass of pass `pass` as run_pass computes it: the blocks and mu / sigma from p (flags and parameters as the pass
 * starts), residuals at (pose, rho, theta) (where its LM loop ended).  Writes, for the flags the pass judges:
 * s_stat[sgood index] = max((r_x scale / w_sx)^2, (r_y scale / w_sy)^2), tf_stat[tfgood index] = max_k |r_k scale / w_t|,
 * tobs_ratio[t] = flagged features / blocks of observation t; entries the pass does not judge are left as they are.
 * thr = (chi2_mono as applied, with +4 when the pass has fewer than 50 text blocks; chi2_text).  Any of the outputs may be NULL. */
int tsba_oracle_outlier_stats(const tsba_problem *p, const tsba_options *o, int pass, const double *pose, const double *rho, const double *theta,
                              double *s_stat, double *tf_stat, double *tobs_ratio, double thr[2]);

/* Full solve (all pyramid passes, outlier passes, write-back into p) -- restates
 * LocalBundleAdjustment / PoseOptim / GlobalBA depending on the options. */
int tsba_oracle_solve(tsba_problem *p, const tsba_options *o, tsba_report *r);

/* mu / sigma of the uint8 intensities inside a projected quad: tool::CalTextinfo + CalStatistics
 * (src/tool.cc:1178-1262) with cv::fillPoly's scan conversion.  corners = 4 x (u,v).
 * Returns 1 if (mu,sigma) valid and sigma != 0, else 0 (sigma is set to 0). */
int tsba_oracle_musigma(const uint8_t *img, int w, int h, const double *corners, double *mu, double *sigma);

/* Rasterised mask of cv::fillPoly (boundary lines + scanline interior) for integer vertices; mask[h*w] in {0,1}. */
void tsba_oracle_fillpoly4(int w, int h, const int *xy, uint8_t *mask);

/* Reduced camera system of the first linearisation of a pass (debug aid for the HIP path):
 *   free_idx [n_kf]       out: column-block index of each KF in S, or -1 (fixed / not participating)
 *   S        [(6nf)^2]    out: Schur complement INCLUDING the LM damping for `radius` (row-major)
 *   g        [6nf]        out: reduced gradient  (b_p - W V^-1 b_l), sign convention: S * dx = -g
 *   Hpp/bp   [(6nf)^2],[6nf] out: undamped pose block and pose gradient (may be NULL)
 *   cost     out: 1/2 sum rho(|r|^2) over non-fixed blocks
 * Returns nf (>=0) or negative error. */
int tsba_oracle_reduced_system(const tsba_problem *p, const tsba_options *o, int level, double radius,
                               int32_t *free_idx, double *S, double *g, double *Hpp, double *bp, double *cost);

/* One rank's contribution to the reduced normal equations of a landmark-sharded global BA (see tsba_oracle.c). */
int tsba_oracle_partial_system(const tsba_problem *p, const tsba_options *o, int level, double radius,
                               int32_t *free_idx, double *S, double *g, double *Hd, double *cost);

/* Covariance of theta[text] (all other parameters constant) at the current parameters, ceres::Covariance semantics. */
/* text label image of a keyframe (optimizer::ShowBAReproj_TextBox -> tool::TextBoxWithFill); out: h*w floats */
int tsba_oracle_label_image(const tsba_problem *p, int kf, int level, float *out);

int tsba_oracle_theta_cov(const tsba_problem *p, const tsba_options *o, int level, int text, double cov[9]);

int tsba_oracle_theta_optim(tsba_problem *p, const tsba_options *o, tsba_report *r, int text, double cov[9]);

/* Reference option sets: kind 0 = LocalBundleAdjustment, 1 = PoseOptim, 2 = GlobalBA. */
void tsba_oracle_default_options(tsba_options *o, int kind);

#ifdef __cplusplus
}
#endif
#endif
