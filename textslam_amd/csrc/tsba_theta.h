// Batched ThetaOptimMultiFs (optimizer::ThetaOptimMultiFs -> PyrThetaOptim, optimizer.cc:565-624,2170-2242; called per immature plane by
// tracking::TextUpdate, tracking.cc:1917-1946): n independent 3-unknown problems, ONE workgroup per plane over all its passes and LM iterations, one launch
// per call.  Included by tsba.hip after tsba_pose.h (tsba_theta_optim_batch there is the host side).
//
// Per pass (level o.levels[p]) a workgroup
//   1. takes mu / sigma of every observing frame at the pass's starting theta (GetProjText + CalTextinfo through musigma_core, the rasteriser the general
//      path's k_musigma runs: the same bits), held constant through the pass as the reference does; a frame with sigma == 0 contributes no blocks
//      (k_linearize's participation rule for its text lanes);
//   2. sweeps the (frame, feature, tap) lanes with text_tap (the general path's and the pose path's device function) and the theta row jl[3], the Huber
//      weight per 8-tap block as pose_sweep_obs applies it, and reduces 10 values (J^T J upper 6, J^T r 3, cost) through LDS in a fixed order;
//   3. takes the Ceres LM decision and the next 3 x 3 trial on thread 0 (theta_step: pose_step of tsba_pose.h restated for one Euclidean 3-vector) and
//      broadcasts the candidate through LDS;
//   4. writes V, the pass's report fields and theta to the plane's output record.
// No workgroup waits for another (no polling, no grid barrier): any residency gives the same bits, and a plane's bits do not depend on its neighbours.
// The constant frame pairs T_cr and the per-frame mu / sigma live in a per-plane scratch record in device memory (17 doubles per observing frame).
#pragma once

#ifndef THETA_WG
#define THETA_WG 256                    /* workgroup size: 256 / 512 / 1024 measured, profiles/theta_batch_timing.txt */
#endif
#define THETA_SCR 18                    /* scratch doubles per observing frame: R_cr 9 | t_q 3 | t_c 3 | mu | sigma | - */

struct ThHdr {                          // one plane, staged by the host
    double K[4];                        // level 0
    double theta[3];                    // start point
    double host[7];                     // pose of the host keyframe
    double box[8];                      // text_box_ray
    int n_obs, o_obs;                   // observing frames: ThObs [o_obs, o_obs + n_obs)
    int nf[TSBA_MAX_LEVELS], o_feat[TSBA_MAX_LEVELS];      // level l: features [o_feat, o_feat + nf) of the uv / ref arrays
    int w[TSBA_MAX_LEVELS], h[TSBA_MAX_LEVELS];
};
struct ThObs { double pose[7]; const uint8_t *img[TSBA_MAX_LEVELS]; };
struct ThOut {                          // one plane, read back by the host
    double theta[3], V[TSBA_MAX_LEVELS][6], cost0[TSBA_MAX_LEVELS], cost1[TSBA_MAX_LEVELS];
    long long evals[TSBA_MAX_LEVELS];   // linearisations + cost evaluations of the pass (tsba_report.n_resid_evals = evals x 8 n_tblock)
    int iters[TSBA_MAX_LEVELS], accepted[TSBA_MAX_LEVELS], term[TSBA_MAX_LEVELS], pad;
};
struct ThArgs { const ThHdr *hdr; const ThObs *obs; const double *fuv, *fref; double *scr; ThOut *out; };

// LM state of one plane (thread 0 of its workgroup)
struct ThState {
    double radius, decrease_factor, x_cost, x_norm, cand_cost, gmax, cost0;
    double M[6], c[3], sig[3], dgs[3], x[3], cand[3], mcc, step2;
    int it, accepted, term, invalid, max_it, done, fail;
    long long evals;
};

// this workgroup's sweep at theta x: thread 0 returns the 10 totals (J^T J upper: xx xy xz yy yz zz | J^T r | cost), fixed summation order
template <int NT>
__device__ __forceinline__ void theta_sweep(const ThObs *obs, const double *scr, const double *fuv, const double *fref, int n_obs, int nf, int l,
                                            const double Kl[4], int w, int hh, const double x[3], const tsba_options &o, double *s_red, double tot[10]) {
    constexpr int NW = NT/64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[10];
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] = 0.0;
    const int nitem = n_obs*nf*8;                            // (a multiple of 8, as NT: the 8 taps of a block sit on 8 neighbouring lanes)
    for (int base = 0; base < nitem; base += NT) {
        const int item = base + tid, kt = item & 7, blk = item >> 3;
        double r = 0.0, jl[3] = { 0.0, 0.0, 0.0 }; bool good = false;
        if (item < nitem) {
            const int t = blk/nf, f = blk - t*nf;
            const double *q = scr + THETA_SCR*t;
            const double sigma = q[16];
            if (sigma != 0.0) {
                good = true;
                PairT T; double tc[3], jt[6];
#pragma unroll
                for (int k = 0; k < 9; k++) T.Rcr[k] = q[k];
#pragma unroll
                for (int k = 0; k < 3; k++) { T.tq[k] = q[9 + k]; tc[k] = q[12 + k]; }
                const double mx = (fuv[2*f] + TAP_DX[kt] - Kl[2])/Kl[0], my = (fuv[2*f+1] + TAP_DY[kt] - Kl[3])/Kl[1];   // tool.cc:1561
                r = text_tap(T, tc, x, mx, my, Kl[0], Kl[1], Kl[2], Kl[3], obs[t].img[l], w, hh, q[15], sigma, 1.0/sigma, fref[8*(size_t)f + kt],
                             o.w_t, true, jt, jl);
            }
        }
        double s8 = r*r;                                     // the block's squared norm
        s8 += __shfl_xor(s8, 1, 64); s8 += __shfl_xor(s8, 2, 64); s8 += __shfl_xor(s8, 4, 64);
        double wgt; const double rho_h = 0.5*huber(s8, o.huber_text, wgt);
        const double wg = good ? wgt : 0.0;
        acc[0] += wg*(jl[0]*jl[0]); acc[1] += wg*(jl[0]*jl[1]); acc[2] += wg*(jl[0]*jl[2]);
        acc[3] += wg*(jl[1]*jl[1]); acc[4] += wg*(jl[1]*jl[2]); acc[5] += wg*(jl[2]*jl[2]);
#pragma unroll
        for (int a = 0; a < 3; a++) acc[6 + a] += wg*(jl[a]*r);
        acc[9] += (good && kt == 0) ? rho_h : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 10; k++) {
        double v = acc[k];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
        acc[k] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 10; k++) s_red[wave*10 + k] = acc[k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 10; k++) { double t = 0.0;
#pragma unroll
            for (int q = 0; q < NW; q++) t += s_red[q*10 + k];
            tot[k] = t; }
    }
    __syncthreads();
}

// sym3 packed upper index: xx xy xz yy yz zz
__device__ __forceinline__ constexpr int sym3(int r, int c) { return r <= c ? r*3 - r*(r - 1)/2 + (c - r) : c*3 - c*(c - 1)/2 + (r - c); }

// One step of the LM state machine on thread 0 -- pose_step of tsba_pose.h (Ceres 1.x TrustRegionMinimizer / LevenbergMarquardtStrategy) restated for
// theta: a Euclidean 3-vector (step2 = |dp|^2, x_norm = |theta|) and a 3 x 3 LDL^T.  tot: the sums of the last sweep; first: the pass's first
// linearisation (Jacobi scaling fixed there, gradient test).  Then the next trial: (M + D/radius) dp = -c and the candidate.
__device__ __forceinline__ void theta_step(ThState &S, const double tot[10], bool first, const tsba_options &o) {
    auto scale = [&](bool fix) {                             // Jacobi scaling fixed at the first linearisation of the pass
#pragma unroll
        for (int q = 0; q < 3; q++) { const double h = S.M[sym3(q, q)]; if (fix) S.sig[q] = 1.0/(1.0 + sqrt(h));
            S.dgs[q] = clampd(S.sig[q]*S.sig[q]*h, o.min_diagonal, o.max_diagonal)/(S.sig[q]*S.sig[q]); }
    };
    auto install = [&]() {                                   // the swept point becomes x
#pragma unroll
        for (int q = 0; q < 6; q++) S.M[q] = tot[q];
        double g = 0.0, v = 0.0;
#pragma unroll
        for (int q = 0; q < 3; q++) { S.c[q] = tot[6 + q]; g = fmax(g, fabs(S.c[q])); v += S.x[q]*S.x[q]; }
        S.gmax = g; S.x_norm = sqrt(v);
    };
    if (first) {
        install(); scale(true);
        S.x_cost = tot[9]; S.cost0 = tot[9]; S.evals++;
        if (S.gmax <= o.gradient_tolerance) { S.done = 1; S.term = 3; }
    } else {
        S.it++;
        const double mcc = 0.5*S.mcc;
        if (S.fail || !(mcc > 0.0)) {                        // invalid step
            if (++S.invalid >= 5) { S.done = 1; S.term = 5; }
            else S.radius *= 0.5;
        } else {
            S.invalid = 0; S.evals++;
            double cost = tot[9]; if (!(cost == cost)) cost = 1.7976931348623157e308;
            S.cand_cost = cost;
            const double cost_change = S.x_cost - cost, step_norm = sqrt(S.step2);
            if (step_norm <= o.parameter_tolerance*(S.x_norm + o.parameter_tolerance)) { S.done = 1; S.term = 2; }
            else if (fabs(cost_change) <= o.function_tolerance*S.x_cost) { S.done = 1; S.term = 1; }
            else {
                const double rel = cost_change/mcc;
                if (rel > o.min_relative_decrease) {
#pragma unroll
                    for (int q = 0; q < 3; q++) S.x[q] = S.cand[q];
                    install(); scale(false); S.accepted++; S.evals++;
                    S.x_cost = cost;
                    double t = 2.0*rel - 1.0, f = 1.0 - t*t*t; if (f < 1.0/3.0) f = 1.0/3.0;
                    S.radius = fmin(S.radius/f, o.max_radius);
                    S.decrease_factor = 2.0;
                    if (S.gmax <= o.gradient_tolerance) { S.done = 1; S.term = 3; }
                } else {
                    S.radius = S.radius/S.decrease_factor; S.decrease_factor *= 2.0;
                }
            }
        }
        if (!S.done) {
            if (S.it >= S.max_it) { S.done = 1; S.term = 0; }
            else if (S.radius < o.min_radius) { S.done = 1; S.term = 4; }
        }
    }
    if (S.done) return;
    // (M + D/radius) dp = -c by LDL^T, candidate, step norm, model cost change
    const double irad = 1.0/S.radius;
    double dp[3] = { 0.0, 0.0, 0.0 }; bool fail = false;
    {
        double s[6];
#pragma unroll
        for (int q = 0; q < 6; q++) s[q] = S.M[q];
        s[0] += S.dgs[0]*irad; s[3] += S.dgs[1]*irad; s[5] += S.dgs[2]*irad;
        // s = L D L^T, L unit lower: d0 = s00; l10 = s01/d0, l20 = s02/d0; d1 = s11 - l10 s01; l21 = (s12 - l10 s02)/d1; d2 = s22 - l20 s02 - l21 (s12 - l10 s02)
        const double d0 = s[0];
        if (!(d0 > 0.0)) fail = true;
        const double id0 = 1.0/d0, l10 = s[1]*id0, l20 = s[2]*id0;
        const double d1 = s[3] - l10*s[1];
        if (!(d1 > 0.0)) fail = true;
        const double e12 = s[4] - l10*s[2], id1 = 1.0/d1, l21 = e12*id1;
        const double d2 = s[5] - l20*s[2] - l21*e12;
        if (!(d2 > 0.0)) fail = true;
        if (!fail) {
            const double z0 = S.c[0], z1 = S.c[1] - l10*z0, z2 = S.c[2] - l20*z0 - l21*z1;
            const double y2 = z2/d2, y1 = z1*id1 - l21*y2, y0 = z0*id0 - l10*y1 - l20*y2;
            dp[0] = -y0; dp[1] = -y1; dp[2] = -y2;
        }
    }
    double step2 = 0.0, mcc = 0.0;
    if (!fail) {
#pragma unroll
        for (int q = 0; q < 3; q++) { S.cand[q] = S.x[q] + dp[q]; step2 += dp[q]*dp[q]; const double lam = S.dgs[q]*irad; mcc += lam*dp[q]*dp[q] - S.c[q]*dp[q]; }
    } else {
#pragma unroll
        for (int q = 0; q < 3; q++) S.cand[q] = S.x[q];
    }
    S.mcc = mcc; S.step2 = step2; S.fail = fail ? 1 : 0;
}

template <int NT>
__global__ __launch_bounds__(NT) void k_theta_batch(ThArgs A, tsba_options o) {
    __shared__ unsigned mask[MS_MASK_WORDS];                 // mu / sigma: the box's polygon mask
    __shared__ unsigned hist[256];
    __shared__ int s_xy[8], s_c[16];
    __shared__ double s_red[NT];                             // mu / sigma moments; the sweep's per-wave sums (NT/64 x 10)
    __shared__ double s_x[3];                                // the point the next sweep is taken at
    __shared__ int s_ctl[2];                                 // done, sweep
    const int tid = threadIdx.x, b = blockIdx.x;
    const ThHdr &H = A.hdr[b];
    const ThObs *obs = A.obs + H.o_obs;
    double *scr = A.scr + THETA_SCR*(size_t)H.o_obs;
    ThOut &out = A.out[b];
    const int n_obs = H.n_obs;
    // the frame pairs T_cr = T_cw T_rw^-1 (every pose is constant)
    for (int t = tid; t < n_obs; t += NT) {
        Pose C, Hs; PairT T;
        load_pose(obs[t].pose, C); load_pose(H.host, Hs); pair_from_poses(C, Hs, T);
        double *q = scr + THETA_SCR*t;
#pragma unroll
        for (int k = 0; k < 9; k++) q[k] = T.Rcr[k];
#pragma unroll
        for (int k = 0; k < 3; k++) { q[9 + k] = T.tq[k]; q[12 + k] = C.t[k]; }
    }
    double x[3] = { H.theta[0], H.theta[1], H.theta[2] };
    ThState S;                                               // (meaningful in thread 0)
    double tot[10];
    for (int ps = 0; ps < o.n_passes; ps++) {
        const int l = o.levels[ps], nf = H.nf[l], w = H.w[l], hh = H.h[l];
        double Kl[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { double v = H.K[k]; for (int q = 0; q < l; q++) v *= 0.5; Kl[k] = v; }
        const double *fuv = A.fuv + 2*(size_t)H.o_feat[l], *fref = A.fref + 8*(size_t)H.o_feat[l];
        // 1. mu / sigma of every observing frame at the pass's starting theta
        {
            double ph[12];
#pragma unroll
            for (int k = 0; k < 12; k++) ph[k] = k < 7 ? H.host[k] : 0.0;
            const double mx = H.box[2*(tid & 3)], my = H.box[2*(tid & 3) + 1];
            for (int t = 0; t < n_obs; t++) {
                double pc[7], mu, sigma;
#pragma unroll
                for (int k = 0; k < 7; k++) pc[k] = obs[t].pose[k];
                musigma_core<NT>(pc, ph, true, x, mx, my, Kl, w, hh, obs[t].img[l], mask, hist, s_xy, s_c, s_red, &mu, &sigma
#ifdef MID_STAMPS
                                 , nullptr, 0
#endif
                                 );
                if (tid == 0) { scr[THETA_SCR*t + 15] = mu; scr[THETA_SCR*t + 16] = sigma; }
            }
            __syncthreads();
        }
        if (tid == 0) {
            S.radius = o.initial_radius; S.decrease_factor = 2.0; S.x_cost = 0.0; S.x_norm = 0.0; S.cand_cost = 0.0; S.gmax = 0.0; S.cost0 = 0.0;
            S.mcc = 0.0; S.step2 = 0.0; S.it = 0; S.accepted = 0; S.term = 0; S.invalid = 0; S.max_it = o.its[ps]; S.done = 0; S.fail = 0; S.evals = 0;
#pragma unroll
            for (int q = 0; q < 3; q++) { S.x[q] = x[q]; S.cand[q] = x[q]; }
        }
        if (n_obs*nf == 0) {                                 // no residual block at all: Ceres has nothing to solve (the oracle's term 5)
            if (tid == 0) { S.done = 1; S.term = 5; for (int q = 0; q < 6; q++) S.M[q] = 0.0; }
        } else {
            // 2. + 3. first linearisation, then one sweep per trial
            theta_sweep<NT>(obs, scr, fuv, fref, n_obs, nf, l, Kl, w, hh, x, o, s_red, tot);
            bool first = true;
            for (;;) {
                if (tid == 0) {
                    theta_step(S, tot, first, o);
                    s_ctl[0] = S.done; s_ctl[1] = !S.done && !S.fail;
#pragma unroll
                    for (int q = 0; q < 3; q++) s_x[q] = S.cand[q];
                }
                first = false;
                __syncthreads();
                const int done = s_ctl[0], sweep = s_ctl[1];
                const double c3[3] = { s_x[0], s_x[1], s_x[2] };
                __syncthreads();
                if (done) break;
                if (sweep) theta_sweep<NT>(obs, scr, fuv, fref, n_obs, nf, l, Kl, w, hh, c3, o, s_red, tot);
            }
        }
        // 4. pass end: V of the last linearisation at x, the report fields; x to every thread for the next pass
        if (tid == 0) {
#pragma unroll
            for (int q = 0; q < 6; q++) out.V[ps][q] = S.M[q];
            out.cost0[ps] = S.cost0; out.cost1[ps] = S.x_cost; out.evals[ps] = S.evals;
            out.iters[ps] = S.it; out.accepted[ps] = S.accepted; out.term[ps] = S.term;
#pragma unroll
            for (int q = 0; q < 3; q++) s_x[q] = S.x[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 3; q++) x[q] = s_x[q];
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 3; q++) out.theta[q] = x[q];
    }
}
