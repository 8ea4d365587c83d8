// libtsloop.so -- loop-closure optimisers on gfx950 (include/tsloop.h).
//
// optimizer::OptimizeSim3 (src/optimizer.cc:626-731): 7 degrees of freedom, a few hundred matches, two 2-row residual blocks per match.
// The whole Levenberg-Marquardt solve is ONE launch of one 256-thread workgroup: the problem is far too small to spread (a sweep is
// one round of ~400 instructions per lane), so the only thing worth optimising is the number of dependent launches -- zero.  Per
// iteration: sweep (residuals, closed-form tangent-space Jacobians, Huber weights; 36 sums = 28 J^T W J + 7 J^T W r + cost through LDS
// transposes), Jacobi-scaled damped 7x7 LDL^T in registers (every thread, redundantly), candidate on the manifold, cost sweep,
// Ceres' accept / reject / radius logic -- then the 4-pixel inlier test of the reference.
// tsloop_sim3_batch (tsloop_ransac.h) runs that solve for every loop candidate in one launch, behind the candidate's Sim3Solver RANSAC.
// tsloop_detect_loop (tsloop_detect.h) is loopClosing::DetectLoop's string scan and keyframe vote: integers and one fp64 quotient per pair.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <chrono>
#include <string>
#include <algorithm>
#include "../../include/tsloop.h"
#include "tsba_device.h"
#include <vector>
#include <map>
#include "tsloop_graph.h"
#include "tsstage.h"

#define SIM_T 256
#define SIM_NW (SIM_T/64)

struct LCtx {
    int device = 0; hipStream_t stream = nullptr; std::string err;
    PinnedBlock h_stage; DeviceBlock d_buf;       // the calls' pinned block and device block, laid out with tsstage.h
    PinnedBlock h_out;                            // tsloop_sim3_batch's pinned block out
};
#define CKL(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { c->err = std::string(#x) + ": " + hipGetErrorString(e_); return TSLOOP_ERR_DEVICE; } } while (0)

struct Sim3Dev { int n; const double *P1, *P2; const float *uv1, *uv2; uint8_t *inlier; double K[4]; double *sim; tsloop_report *rep; };

// residuals (4) and tangent-space Jacobians (4 x 7: delta(3) | t(3) | s) of one match.  Ceres' quaternion Plus perturbs on the left with
// the half angle: R+ = Exp(2 delta) R.
//   auto_sim    X = s R P2 + t:        dX/ddelta = -2 [s R P2]x,   dX/dt = I,        dX/ds = R P2
//   auto_siminv Y = R^T (P1 - t) / s:  dY/ddelta = (2/s) R^T [P1 - t]x,  dY/dt = -R^T / s,  dY/ds = -Y / s
__device__ __forceinline__ void sim3_match(const double R[9], const double t[3], double s, const double P1[3], const double P2[3],
                                           double u1, double v1, double u2, double v2, const double K[4], bool want_j, double r[4], double J[4][7]) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    {
        double A[3]; mat3_vec(R, P2, A);
        const double sA[3] = { s*A[0], s*A[1], s*A[2] };
        const double X = sA[0] + t[0], Y = sA[1] + t[1], Z = sA[2] + t[2], iz = 1.0/Z;
        r[0] = X*iz*fx + cx - u1; r[1] = Y*iz*fy + cy - v1;
        if (want_j) {
            const double d0[3] = { fx*iz, 0.0, -fx*X*iz*iz }, d1[3] = { 0.0, fy*iz, -fy*Y*iz*iz };
            // row * (-2 [sA]x): (d x sA)-type products; [v]x = [[0,-vz,vy],[vz,0,-vx],[-vy,vx,0]]
            J[0][0] = -2.0*(d0[1]*sA[2] - d0[2]*sA[1]); J[0][1] = -2.0*(d0[2]*sA[0] - d0[0]*sA[2]); J[0][2] = -2.0*(d0[0]*sA[1] - d0[1]*sA[0]);
            J[1][0] = -2.0*(d1[1]*sA[2] - d1[2]*sA[1]); J[1][1] = -2.0*(d1[2]*sA[0] - d1[0]*sA[2]); J[1][2] = -2.0*(d1[0]*sA[1] - d1[1]*sA[0]);
#pragma unroll
            for (int k = 0; k < 3; k++) { J[0][3 + k] = d0[k]; J[1][3 + k] = d1[k]; }
            J[0][6] = d0[0]*A[0] + d0[2]*A[2]; J[1][6] = d1[1]*A[1] + d1[2]*A[2];
        }
    }
    {
        const double D[3] = { P1[0] - t[0], P1[1] - t[1], P1[2] - t[2] }, is = 1.0/s;
        double E[3]; mat3T_vec(R, D, E);
        const double X = E[0]*is, Y = E[1]*is, Z = E[2]*is, iz = 1.0/Z;
        r[2] = X*iz*fx + cx - u2; r[3] = Y*iz*fy + cy - v2;
        if (want_j) {
            const double d0[3] = { fx*iz, 0.0, -fx*X*iz*iz }, d1[3] = { 0.0, fy*iz, -fy*Y*iz*iz };
            // g = R d (so that d^T R^T M = (R d)^T M); d^T (2/s) R^T [D]x = (2/s) (g x D)^T ... with [D]x v = D x v: g^T [D]x = (g x D)^T
            double g0[3], g1[3]; mat3_vec(R, d0, g0); mat3_vec(R, d1, g1);
            const double c2 = 2.0*is;
            J[2][0] = c2*(g0[1]*D[2] - g0[2]*D[1]); J[2][1] = c2*(g0[2]*D[0] - g0[0]*D[2]); J[2][2] = c2*(g0[0]*D[1] - g0[1]*D[0]);
            J[3][0] = c2*(g1[1]*D[2] - g1[2]*D[1]); J[3][1] = c2*(g1[2]*D[0] - g1[0]*D[2]); J[3][2] = c2*(g1[0]*D[1] - g1[1]*D[0]);
#pragma unroll
            for (int k = 0; k < 3; k++) { J[2][3 + k] = -g0[k]*is; J[3][3 + k] = -g1[k]*is; }
            J[2][6] = -(d0[0]*X + d0[2]*Z)*is; J[3][6] = -(d1[1]*Y + d1[2]*Z)*is;
        }
    }
}

// sums of NV <= 18 per-thread values over the workgroup: thread v < NV returns the total (fixed order: deterministic)
template <int NV>
__device__ __forceinline__ double wg_sum_to_lane(const double *acc, double *lds /* SIM_NW*18*65 + SIM_NW*32 */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *reg = lds + wave*18*65, *xw = lds + SIM_NW*18*65;
#pragma unroll
    for (int i = 0; i < NV; i++) reg[i*65 + lane] = acc[i];
    __syncthreads();
    if (lane < NV) {
        const double *row = reg + lane*65;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int q = 0; q < 64; q += 4) { s0 += row[q]; s1 += row[q + 1]; s2 += row[q + 2]; s3 += row[q + 3]; }
        xw[wave*32 + lane] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    double tot = 0.0;
    if (tid < NV) {
#pragma unroll
        for (int w = 0; w < SIM_NW; w++) tot += xw[w*32 + tid];
    }
    __syncthreads();
    return tot;
}

__device__ __forceinline__ constexpr int sym7(int r, int c) { return r <= c ? r*7 - r*(r - 1)/2 + (c - r) : c*7 - c*(c - 1)/2 + (r - c); }

#define SIM_LDS_DOUBLES (SIM_NW*18*65 + SIM_NW*32)
// The whole LM solve of one Sim3 problem by the calling workgroup (SIM_T threads; lds: SIM_LDS_DOUBLES, s_tot: 40 doubles of LDS).  k_sim3_lm runs it on
// the one problem of tsloop_optimize_sim3, k_sim3_batch (tsloop_ransac.h) on each candidate's slice after its RANSAC: one statement of the arithmetic.
__device__ __forceinline__ void sim3_lm_body(const Sim3Dev P, const tsloop_options o, double *lds, double *s_tot) {
    const int tid = threadIdx.x;
    double x[8];
    {   const double n = sqrt(P.sim[0]*P.sim[0] + P.sim[1]*P.sim[1] + P.sim[2]*P.sim[2] + P.sim[3]*P.sim[3]);      // q = q.normalized(), optimizer.cc:639
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = P.sim[k]/n;
#pragma unroll
        for (int k = 4; k < 8; k++) x[k] = P.sim[k]; }
    // full = true: M (28, upper, sym7 order), c (7), cost -> s_tot[0..35]; false: cost only -> s_tot[35].  All threads get them.
    auto sweep = [&](const double *xx, bool full) {
        double R[9]; quat_to_R(xx, R);
        double acc[36];
#pragma unroll
        for (int k = 0; k < 36; k++) acc[k] = 0.0;
#pragma unroll 1
        for (int i = tid; i < P.n; i += SIM_T) {
            if (!P.inlier[i]) continue;
            const double P1[3] = { P.P1[3*i], P.P1[3*i+1], P.P1[3*i+2] }, P2[3] = { P.P2[3*i], P.P2[3*i+1], P.P2[3*i+2] };
            double r[4], J[4][7];
            sim3_match(R, xx + 4, xx[7], P1, P2, (double)P.uv1[2*i], (double)P.uv1[2*i+1], (double)P.uv2[2*i], (double)P.uv2[2*i+1], P.K, full, r, J);
#pragma unroll
            for (int b = 0; b < 2; b++) {                             // one robust weight per residual block
                double w; acc[35] += 0.5*huber(r[2*b]*r[2*b] + r[2*b+1]*r[2*b+1], o.huber_delta, w);
                if (full) {
                    int q = 0;
#pragma unroll
                    for (int a = 0; a < 7; a++)
#pragma unroll
                        for (int cc = a; cc < 7; cc++) { acc[q] += w*(J[2*b][a]*J[2*b][cc] + J[2*b+1][a]*J[2*b+1][cc]); q++; }
#pragma unroll
                    for (int a = 0; a < 7; a++) acc[28 + a] += w*(J[2*b][a]*r[2*b] + J[2*b+1][a]*r[2*b+1]);
                }
            }
        }
        if (full) {
            const double t0 = wg_sum_to_lane<18>(acc, lds), t1 = wg_sum_to_lane<18>(acc + 18, lds);
            if (tid < 18) { s_tot[tid] = t0; s_tot[18 + tid] = t1; }
        } else {
            const double t1 = wg_sum_to_lane<1>(acc + 35, lds);
            if (tid == 0) s_tot[35] = t1;
        }
        __syncthreads();
    };
    int nact = 0;
    for (int i = 0; i < P.n; i++) nact += P.inlier[i] ? 1 : 0;          // (uniform, tiny)
    double M[28], c[7], sc[7], x_cost, x_norm;
    auto install = [&]() {
#pragma unroll
        for (int k = 0; k < 28; k++) M[k] = s_tot[k];
#pragma unroll
        for (int k = 0; k < 7; k++) c[k] = s_tot[28 + k];
        x_cost = s_tot[35];
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) v += x[k]*x[k];
        x_norm = sqrt(v);
        __syncthreads();
    };
    sweep(x, true); install();
#pragma unroll
    for (int k = 0; k < 7; k++) sc[k] = 1.0/(1.0 + sqrt(M[sym7(k, k)]));
    const double cost0 = x_cost;
    double radius = o.initial_radius, decrease_factor = 2.0; int invalid = 0, term = 0, it = 0, accepted = 0;
    auto gmax_of = [&]() { double g = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) g = fmax(g, fabs(c[k])); return g; };
    bool stop = false;
    if (nact == 0) { term = 5; stop = true; }
    else if (gmax_of() <= o.gradient_tolerance) { term = 3; stop = true; }
    while (!stop) {
        if (it >= o.max_it) { term = 0; break; }
        if (radius < o.min_radius) { term = 4; break; }
        it++;
        // (S M S + D / radius) y = -S c, LDL^T without pivoting (positive definite by construction), d = S y
        double A[28], y[7], d[7]; bool bad = false;
#pragma unroll
        for (int a = 0; a < 7; a++)
#pragma unroll
            for (int b = a; b < 7; b++) A[sym7(a, b)] = sc[a]*M[sym7(a, b)]*sc[b];
#pragma unroll
        for (int a = 0; a < 7; a++) { const double dg = fmin(fmax(sc[a]*sc[a]*M[sym7(a, a)], o.min_diagonal), o.max_diagonal); A[sym7(a, a)] += dg/radius; y[a] = -sc[a]*c[a]; }
        double L[7][7], dd[7];
#pragma unroll
        for (int j = 0; j < 7; j++) {
            double v = A[sym7(j, j)];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[j][k]*L[j][k]*dd[k];
            if (!(v > 0.0)) { bad = true; v = 1.0; }
            dd[j] = v;
#pragma unroll
            for (int i = j + 1; i < 7; i++) { double u = A[sym7(j, i)];
#pragma unroll
                for (int k = 0; k < j; k++) u -= L[i][k]*L[j][k]*dd[k];
                L[i][j] = u/v; }
        }
#pragma unroll
        for (int i = 0; i < 7; i++) {
#pragma unroll
            for (int k = 0; k < i; k++) y[i] -= L[i][k]*y[k]; }
#pragma unroll
        for (int i = 0; i < 7; i++) y[i] /= dd[i];
#pragma unroll
        for (int i = 6; i >= 0; i--) {
#pragma unroll
            for (int k = i + 1; k < 7; k++) y[i] -= L[k][i]*y[k]; }
        double model_change = -1.0;
        if (!bad) {
#pragma unroll
            for (int k = 0; k < 7; k++) d[k] = sc[k]*y[k];
            model_change = 0.0;                                        // -(J d)^T (r + J d / 2) = -d^T (c + M d / 2)
#pragma unroll
            for (int k = 0; k < 7; k++) { double hd = 0.0;
#pragma unroll
                for (int m = 0; m < 7; m++) hd += M[sym7(k, m)]*d[m];
                model_change -= d[k]*(c[k] + 0.5*hd); }
        }
        if (bad || !(model_change > 0.0)) { if (++invalid >= 5) { term = 5; break; } radius *= 0.5; continue; }
        invalid = 0;
        double cand[8];
        quat_plus(x, d, cand);
#pragma unroll
        for (int k = 0; k < 4; k++) cand[4 + k] = x[4 + k] + d[3 + k];
        sweep(cand, true);                                             // speculative: the linearisation at the candidate (cost in s_tot[35])
        double c_cost = s_tot[35]; if (!(c_cost == c_cost)) c_cost = 1.7976931348623157e308;
        double step = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) step += (cand[k] - x[k])*(cand[k] - x[k]);
        step = sqrt(step);
        if (step <= o.parameter_tolerance*(x_norm + o.parameter_tolerance)) { term = 2; break; }
        const double cost_change = x_cost - c_cost;
        if (fabs(cost_change) <= o.function_tolerance*x_cost) { term = 1; break; }
        const double rel = cost_change/model_change;
        if (rel > o.min_relative_decrease) {
#pragma unroll
            for (int k = 0; k < 8; k++) x[k] = cand[k];
            install(); accepted++;
            double t = 2.0*rel - 1.0, f = 1.0 - t*t*t; if (f < 1.0/3.0) f = 1.0/3.0;
            radius = fmin(radius/f, o.max_radius); decrease_factor = 2.0;
            if (gmax_of() <= o.gradient_tolerance) { term = 3; break; }
        } else { radius = radius/decrease_factor; decrease_factor *= 2.0; __syncthreads(); }
    }
    __syncthreads();
    // result (q12.normalized()) and the inlier test, optimizer.cc:682-729
    {   const double n = sqrt(x[0]*x[0] + x[1]*x[1] + x[2]*x[2] + x[3]*x[3]);
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = x[k]/n; }
    double R[9]; quat_to_R(x, R);
    int ninl = 0;
    for (int i = tid; i < P.n; i += SIM_T) {
        if (!P.inlier[i]) continue;
        const double P1[3] = { P.P1[3*i], P.P1[3*i+1], P.P1[3*i+2] }, P2[3] = { P.P2[3*i], P.P2[3*i+1], P.P2[3*i+2] };
        double r[4], J[4][7];
        sim3_match(R, x + 4, x[7], P1, P2, (double)P.uv1[2*i], (double)P.uv1[2*i+1], (double)P.uv2[2*i], (double)P.uv2[2*i+1], P.K, false, r, J);
        if (fabs(r[0]) >= o.thresh_outlier || fabs(r[1]) >= o.thresh_outlier || fabs(r[2]) >= o.thresh_outlier || fabs(r[3]) >= o.thresh_outlier) P.inlier[i] = 0;
        else ninl++;
    }
    double nv = (double)ninl;
    const double tot = wg_sum_to_lane<1>(&nv, lds);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) P.sim[k] = x[k];
        P.rep->iters = it; P.rep->accepted = accepted; P.rep->termination = term; P.rep->n_inlier = (int)tot; P.rep->cost0 = cost0; P.rep->cost1 = x_cost;
    }
}

__global__ __launch_bounds__(SIM_T) void k_sim3_lm(Sim3Dev P, tsloop_options o) {
    __shared__ double lds[SIM_LDS_DOUBLES];
    __shared__ double s_tot[40];
    sim3_lm_body(P, o, lds, s_tot);
}

#include "tsloop_ransac.h"
#include "tsloop_detect.h"

// ------------------------------------------------------------------------------------------------ host side
extern "C" {

void tsloop_default_options_sim3(tsloop_options *o) {
    memset(o, 0, sizeof(*o));
    o->max_it = 20; o->huber_delta = sqrt(10.0); o->thresh_outlier = 4.0;
    o->initial_radius = 1e4; o->max_radius = 1e16; o->min_radius = 1e-32; o->min_relative_decrease = 1e-3;
    o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8; o->min_diagonal = 1e-6; o->max_diagonal = 1e32;
}
int tsloop_create(int device, void **ctx) {
    if (!ctx) return TSLOOP_ERR_ARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return TSLOOP_ERR_DEVICE;       // no GPU: fail loudly, no CPU path
    LCtx *c = new LCtx(); c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess) { delete c; return TSLOOP_ERR_DEVICE; }
    *ctx = c; return TSLOOP_OK;
}
void tsloop_destroy(void *ctx) {
    LCtx *c = (LCtx *)ctx; if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    delete c;                               // the blocks go with the context
}
const char *tsloop_last_error(void *ctx) { LCtx *c = (LCtx *)ctx; return c ? c->err.c_str() : "null context"; }

int tsloop_optimize_sim3(void *ctx, tsloop_sim3_problem *p, const tsloop_options *o, tsloop_report *r) {
    LCtx *c = (LCtx *)ctx;
    if (!c || !p || !o || !r || p->n < 0 || (p->n > 0 && (!p->P1 || !p->P2 || !p->uv1 || !p->uv2 || !p->inlier))) return TSLOOP_ERR_ARG;
    if (!(p->sim[7] > 0.0)) { c->err = "scale must be positive"; return TSLOOP_ERR_ARG; }
    hipSetDevice(c->device);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = (size_t)p->n;
    // in: [P1 | P2 | uv1 | uv2]   in and out: [sim | rep | inlier]
    Layout L(256);
    const auto a_P1 = L.take<double>(3*n), a_P2 = L.take<double>(3*n); const auto a_u1 = L.take<float>(2*n), a_u2 = L.take<float>(2*n);
    const auto a_sim = L.take<double>(8); const auto a_rep = L.take<tsloop_report>(1); const auto a_inl = L.take<uint8_t>(n);
    CKL(c->h_stage.grow(L.mark())); CKL(c->d_buf.grow(L.mark()));
    void *h = c->h_stage.as(), *d = c->d_buf.as();
    a_P1.put(h, p->P1); a_P2.put(h, p->P2); a_u1.put(h, p->uv1); a_u2.put(h, p->uv2);
    a_sim.put(h, p->sim); memset(a_rep.at(h), 0, a_rep.bytes()); a_inl.put(h, p->inlier);
    CKL(hipMemcpyAsync(d, h, L.mark(), hipMemcpyHostToDevice, c->stream));            // one staged copy in, one out
    Sim3Dev D; D.n = p->n; D.P1 = a_P1.at(d); D.P2 = a_P2.at(d); D.uv1 = a_u1.at(d); D.uv2 = a_u2.at(d);
    D.inlier = a_inl.at(d); memcpy(D.K, p->K, sizeof(D.K)); D.sim = a_sim.at(d); D.rep = a_rep.at(d);
    hipLaunchKernelGGL(k_sim3_lm, dim3(1), dim3(SIM_T), 0, c->stream, D, *o);
    CKL(hipMemcpyAsync(a_sim.at(h), a_sim.at(d), L.mark() - a_sim.off, hipMemcpyDeviceToHost, c->stream));
    CKL(hipStreamSynchronize(c->stream)); CKL(hipGetLastError());
    a_sim.get(h, p->sim); a_rep.get(h, r); a_inl.get(h, p->inlier);
    r->t_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return r->termination == 5 ? TSLOOP_ERR_NUMERIC : TSLOOP_OK;
}

void tsloop_default_options_sim3_ransac(tsloop_sim3_batch_problem *p) { p->min_inliers = 20; p->max_err2 = 45.0; p->optimise = 1; }

int tsloop_sim3_batch(void *ctx, tsloop_sim3_batch_problem *p, const tsloop_options *o) {
    LCtx *c = (LCtx *)ctx;
    if (!c) return TSLOOP_ERR_ARG;
    auto bad = [&](const char *what) { c->err = std::string("tsloop_sim3_batch: ") + what; return TSLOOP_ERR_ARG; };
    if (!p || !o) return bad("NULL problem or options");
    if (p->n_cand < 0) return bad("negative n_cand");
    if (p->n_cand == 0) return TSLOOP_OK;
    const int nc = p->n_cand;
    if (!p->off || !p->hyp_off || !p->K2 || !p->ok || !p->sel || !p->n_inlier_ransac || !p->sim_ransac) return bad("NULL pointer");
    if (p->optimise && (!p->sim || !p->rep)) return bad("NULL sim or rep with optimise");
    if (p->off[0] != 0 || p->hyp_off[0] != 0) return bad("offsets do not start at 0");
    for (int k = 0; k < nc; k++) {
        if (p->off[k + 1] < p->off[k] || p->hyp_off[k + 1] < p->hyp_off[k]) return bad("offsets decrease");
        if (p->hyp_off[k + 1] - p->hyp_off[k] > TSLOOP_RANSAC_MAX_HYP) return bad("more than TSLOOP_RANSAC_MAX_HYP hypotheses of a candidate");
    }
    const size_t n = (size_t)p->off[nc], nh = (size_t)p->hyp_off[nc];
    if (n > (size_t)INT32_MAX/3) return bad("more matches than the kernels index (3 n must fit an int32)");
    if (n > 0 && (!p->P1 || !p->P2 || !p->pred1 || !p->pred2 || !p->uv1 || !p->uv2 || !p->inlier)) return bad("NULL match array");
    if (nh > 0 && !p->triple) return bad("NULL triple");
    if (p->min_inliers < 0) return bad("min_inliers < 0");
    if (!std::isfinite(p->max_err2) || p->max_err2 < 0.0) return bad("max_err2 not finite or negative");
    std::vector<int32_t> act;
    for (int k = 0; k < nc; k++) {
        const int nk = p->off[k + 1] - p->off[k];
        for (int h = p->hyp_off[k]; h < p->hyp_off[k + 1]; h++) {
            const int32_t *t = p->triple + 3*(size_t)h;
            if (t[0] < 0 || t[0] >= nk || t[1] < 0 || t[1] >= nk || t[2] < 0 || t[2] >= nk) return bad("triple index outside the candidate");
            if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) return bad("equal indices in a triple");
        }
        if (p->hyp_off[k + 1] > p->hyp_off[k]) act.push_back(k);
    }
    {   bool fin = true;
        for (int j = 0; j < 4; j++) fin = fin && std::isfinite(p->K1[j]) && std::isfinite(p->K[j]);
        for (size_t j = 0; j < 4*(size_t)nc; j++) fin = fin && std::isfinite(p->K2[j]);
        for (size_t j = 0; j < 3*n; j++) fin = fin && std::isfinite(p->P1[j]) && std::isfinite(p->P2[j]);
        for (size_t j = 0; j < 2*n; j++) fin = fin && std::isfinite(p->pred1[j]) && std::isfinite(p->pred2[j]) && std::isfinite(p->uv1[j]) && std::isfinite(p->uv2[j]);
        if (!fin) return bad("non-finite P, pred, uv or K"); }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t na = act.size();
    // a candidate without hypotheses (N < mRansacMinInliers, Sim3Solver.cc:65-69) is answered here: not ok, nothing selected, no work of its own
    auto fill_idle = [&]() {
        for (int k = 0; k < nc; k++) if (p->hyp_off[k + 1] == p->hyp_off[k]) {
            p->ok[k] = 0; p->sel[k] = -1; p->n_inlier_ransac[k] = 0; memset(p->sim_ransac + 8*(size_t)k, 0, 64);
            if (p->off[k + 1] > p->off[k]) memset(p->inlier + p->off[k], 0, (size_t)(p->off[k + 1] - p->off[k]));
        } };
    if (na == 0) { fill_idle(); return TSLOOP_OK; }
    hipSetDevice(c->device);
    // in: [cand | off | hyp_off | triple | K2 | P1 | P2 | pred1 | pred2 | uv1 | uv2]   out, behind it on the device and in a pinned block of its own:
    // [ok | sel | n_inlier | hyp_count | sim_ransac | sim | hyp_sim | rep | inlier]
    const size_t NC = (size_t)nc;
    Layout L(256), Lo(256);
    const auto a_cand = L.take<int32_t>(na), a_off = L.take<int32_t>(NC + 1), a_hoff = L.take<int32_t>(NC + 1), a_tri = L.take<int32_t>(3*nh);
    const auto a_K2 = L.take<double>(4*NC), a_P1 = L.take<double>(3*n), a_P2 = L.take<double>(3*n), a_q1 = L.take<double>(2*n), a_q2 = L.take<double>(2*n);
    const auto a_u1 = L.take<float>(2*n), a_u2 = L.take<float>(2*n);
    const auto a_ok = Lo.take<int32_t>(NC), a_sel = Lo.take<int32_t>(NC), a_ni = Lo.take<int32_t>(NC), a_hc = Lo.take<int32_t>(nh);
    const auto a_sr = Lo.take<double>(8*NC), a_sim = Lo.take<double>(8*NC), a_hs = Lo.take<double>(8*nh); const auto a_rep = Lo.take<tsloop_report>(NC); const auto a_inl = Lo.take<uint8_t>(n);
    CKL(c->h_stage.grow(L.mark())); CKL(c->h_out.grow(Lo.mark())); CKL(c->d_buf.grow(L.mark() + Lo.mark()));
    void *h = c->h_stage.as(), *d = c->d_buf.as(), *dout = (uint8_t *)d + L.mark(); const void *ho = c->h_out.as();
    a_cand.put(h, act.data()); a_off.put(h, p->off); a_hoff.put(h, p->hyp_off); a_tri.put(h, p->triple); a_K2.put(h, p->K2);
    a_P1.put(h, p->P1); a_P2.put(h, p->P2); a_q1.put(h, p->pred1); a_q2.put(h, p->pred2); a_u1.put(h, p->uv1); a_u2.put(h, p->uv2);
    CKL(hipMemcpyAsync(d, h, L.mark(), hipMemcpyHostToDevice, c->stream));                          // one copy in, one launch, one copy out
    Sim3BatchDev B;
    B.cand = a_cand.at(d); B.off = a_off.at(d); B.hyp_off = a_hoff.at(d); B.triple = a_tri.at(d);
    B.P1 = a_P1.at(d); B.P2 = a_P2.at(d); B.pred1 = a_q1.at(d); B.pred2 = a_q2.at(d); B.uv1 = a_u1.at(d); B.uv2 = a_u2.at(d); B.K2 = a_K2.at(d);
    memcpy(B.K1, p->K1, sizeof(B.K1)); memcpy(B.K, p->K, sizeof(B.K)); B.max_err2 = p->max_err2; B.min_inliers = p->min_inliers; B.optimise = p->optimise ? 1 : 0;
    B.ok = a_ok.at(dout); B.sel = a_sel.at(dout); B.ninl = a_ni.at(dout); B.hyp_count = a_hc.at(dout);
    B.sim_ransac = a_sr.at(dout); B.sim = a_sim.at(dout); B.hyp_sim = a_hs.at(dout); B.rep = a_rep.at(dout); B.inlier = a_inl.at(dout);
    hipLaunchKernelGGL(k_sim3_batch, dim3((unsigned)na), dim3(SIM_T), 0, c->stream, B, *o);
    CKL(hipMemcpyAsync(c->h_out.as(), dout, Lo.mark(), hipMemcpyDeviceToHost, c->stream));
    CKL(hipStreamSynchronize(c->stream)); CKL(hipGetLastError());
    const double t_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fill_idle();
    int rc = TSLOOP_OK;
    for (size_t a = 0; a < na; a++) {
        const size_t k = (size_t)act[a];
        const int ok = a_ok.at(ho)[k];
        p->ok[k] = ok ? 1 : 0; p->sel[k] = a_sel.at(ho)[k]; p->n_inlier_ransac[k] = a_ni.at(ho)[k];
        std::copy_n(a_sr.at(ho) + 8*k, 8, p->sim_ransac + 8*k);
        std::copy(a_inl.at(ho) + p->off[k], a_inl.at(ho) + p->off[k + 1], p->inlier + p->off[k]);
        if (ok && p->optimise) {
            std::copy_n(a_sim.at(ho) + 8*k, 8, p->sim + 8*k); p->rep[k] = a_rep.at(ho)[k];
            p->rep[k].t_ms = t_ms;
            if (p->rep[k].termination == 5) rc = TSLOOP_ERR_NUMERIC;
        }
    }
    a_hc.get(ho, p->hyp_count); a_hs.get(ho, p->hyp_sim);
    return rc;
}

void tsloop_default_options_detect(tsloop_detect_problem *p) { p->min_str_score = 0.3; p->score_thresh_min = 0.51; p->top_n = 10; p->max_match = 64; }

int tsloop_detect_loop(void *ctx, tsloop_detect_problem *p) {
    LCtx *c = (LCtx *)ctx;
    if (!c) return TSLOOP_ERR_ARG;
    auto bad = [&](const char *what) { c->err = std::string("tsloop_detect_loop: ") + what; return TSLOOP_ERR_ARG; };
    if (!p) return bad("NULL problem");
    if (p->n_query < 0 || p->n_map < 0 || p->n_kf < 0) return bad("negative count");
    if (p->top_n < 1) return bad("top_n < 1");
    if (p->max_match < 1) return bad("max_match < 1");
    if (p->min_matched_words < 0) return bad("min_matched_words < 0");
    if (!std::isfinite(p->min_str_score) || !std::isfinite(p->score_thresh_min)) return bad("non-finite threshold");
    const size_t nq = (size_t)p->n_query, nm = (size_t)p->n_map, nk = (size_t)p->n_kf, mm = (size_t)p->max_match;
    auto no_votes = [&]() { if (p->kf_score) memset(p->kf_score, 0, 4*nk); if (p->kf_nobj) memset(p->kf_nobj, 0, 4*nk); if (p->n_cand) *p->n_cand = 0; };
    if (nq == 0) { no_votes(); return TSLOOP_OK; }                      // no query: no input is read, the vote is empty
    if (!p->match_cnt || !p->match_idx || !p->match_dist || !p->match_score || !p->n_cand || !p->cand || (nk > 0 && (!p->kf_score || !p->kf_nobj))) return bad("NULL output pointer");
    if (nm == 0) { memset(p->match_cnt, 0, 4*nq); no_votes(); return TSLOOP_OK; }
    if (!p->q_off || !p->q_self || !p->m_off || !p->m_skip || !p->obs_off) return bad("NULL input pointer");
    if (p->q_off[0] != 0 || p->m_off[0] != 0 || p->obs_off[0] != 0) return bad("offsets do not start at 0");
    for (size_t q = 0; q < nq; q++) {
        if (p->q_off[q + 1] < p->q_off[q]) return bad("q_off decreases");
        if (p->q_off[q + 1] - p->q_off[q] > TSLOOP_TEXT_MAX_LEN) return bad("a query string longer than TSLOOP_TEXT_MAX_LEN");
        if (p->q_self[q] < -1 || p->q_self[q] >= p->n_map) return bad("q_self outside [-1, n_map)");
    }
    for (size_t m = 0; m < nm; m++) {
        if (p->m_off[m + 1] < p->m_off[m] || p->obs_off[m + 1] < p->obs_off[m]) return bad("m_off or obs_off decreases");
        if (p->m_off[m + 1] - p->m_off[m] > TSLOOP_TEXT_MAX_LEN) return bad("a map string longer than TSLOOP_TEXT_MAX_LEN");
    }
    const size_t qb = (size_t)p->q_off[nq], mb = (size_t)p->m_off[nm], no = (size_t)p->obs_off[nm];
    if ((qb > 0 && !p->q_str) || (mb > 0 && !p->m_str) || (no > 0 && !p->obs_kf)) return bad("NULL q_str, m_str or obs_kf");
    for (size_t m = 0; m < nm; m++)
        for (int e = p->obs_off[m]; e < p->obs_off[m + 1]; e++) {
            if (p->obs_kf[e] < 0 || p->obs_kf[e] >= p->n_kf) return bad("obs_kf outside [0, n_kf)");
            if (e > p->obs_off[m] && p->obs_kf[e] <= p->obs_kf[e - 1]) return bad("obs_kf not strictly increasing in its row");
        }
    const size_t n_tile = (nm + TD_T - 1)/TD_T;
    if (n_tile*nq > (size_t)INT32_MAX) return bad("more (query, tile of map texts) pairs than a grid holds");
    hipSetDevice(c->device);
    const size_t nsel = std::min((size_t)p->top_n, nk);
    // in: [q_off | q_str | q_self | m_off | m_str | m_skip | obs_off | obs_kf]   scratch: [dist | hit | tmp_idx | tmp_score | rank_rec]
    // out, behind it on the device and in a pinned block of its own: [match_cnt | rec_off | kf_score | kf_nobj | n_cand | cand | out_rec]
    Layout L(256), Lo(256);
    const auto a_qoff = L.take<int32_t>(nq + 1); const auto a_qstr = L.take<uint8_t>(qb); const auto a_qself = L.take<int32_t>(nq), a_moff = L.take<int32_t>(nm + 1);
    const auto a_mstr = L.take<uint8_t>(mb), a_mskip = L.take<uint8_t>(nm); const auto a_ooff = L.take<int32_t>(nm + 1), a_okf = L.take<int32_t>(no);
    const size_t in_end = L.mark();
    const auto a_dist = L.take<uint8_t>(nq*nm); const auto a_hit = L.take<int32_t>(nm), a_tidx = L.take<int32_t>(nq*mm); const auto a_tsc = L.take<double>(nq*mm); const auto a_rrec = L.take<TdRec>(nq*mm);
    const auto a_cnt = Lo.take<int32_t>(nq), a_roff = Lo.take<int32_t>(nq + 1), a_ks = Lo.take<int32_t>(nk), a_ko = Lo.take<int32_t>(nk), a_nc = Lo.take<int32_t>(1), a_cand = Lo.take<int32_t>(nsel);
    const auto a_rec = Lo.take<TdRec>(nq*mm);
    // the packed lists come last: the one copy out takes as many records as the default capacity holds, a second one only what lies beyond them
    const size_t n_first = nq*std::min(mm, (size_t)64), out_sz = a_rec.off + sizeof(TdRec)*n_first;
    CKL(c->h_stage.grow(in_end)); CKL(c->h_out.grow(out_sz)); CKL(c->d_buf.grow(L.mark() + Lo.mark()));
    void *h = c->h_stage.as(), *d = c->d_buf.as(), *dout = (uint8_t *)d + L.mark(); const void *ho = c->h_out.as();
    a_qoff.put(h, p->q_off); a_qstr.put(h, p->q_str); a_qself.put(h, p->q_self); a_moff.put(h, p->m_off); a_mstr.put(h, p->m_str); a_mskip.put(h, p->m_skip);
    a_ooff.put(h, p->obs_off); a_okf.put(h, p->obs_kf);
    CKL(hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, c->stream));                            // one copy in, three launches, one copy out (two after a max_match above the default)
    TdDev D;
    D.n_query = p->n_query; D.n_map = p->n_map; D.n_kf = p->n_kf; D.top_n = p->top_n; D.n_tile = (int32_t)n_tile; D.max_match = p->max_match; D.min_matched_words = p->min_matched_words;
    D.q_off = a_qoff.at(d); D.q_str = a_qstr.at(d); D.q_self = a_qself.at(d); D.m_off = a_moff.at(d); D.m_str = a_mstr.at(d); D.m_skip = a_mskip.at(d);
    D.obs_off = a_ooff.at(d); D.obs_kf = a_okf.at(d);
    D.min_str_score = p->min_str_score; D.score_thresh_min = p->score_thresh_min;
    D.dist = a_dist.at(d); D.hit = a_hit.at(d); D.tmp_idx = a_tidx.at(d); D.tmp_score = a_tsc.at(d); D.rank_rec = a_rrec.at(d);
    D.match_cnt = a_cnt.at(dout); D.rec_off = a_roff.at(dout); D.out_rec = a_rec.at(dout);
    D.kf_score = a_ks.at(dout); D.kf_nobj = a_ko.at(dout); D.n_cand = a_nc.at(dout); D.cand = a_cand.at(dout);
    hipLaunchKernelGGL(k_td_scan, dim3((unsigned)(n_tile*nq)), dim3(TD_T), 0, c->stream, D);
    hipLaunchKernelGGL(k_td_pick, dim3((unsigned)nq), dim3(TD_T), 0, c->stream, D);
    hipLaunchKernelGGL(k_td_vote, dim3(1), dim3(TD_T), 0, c->stream, D);
    CKL(hipMemcpyAsync(c->h_out.as(), dout, out_sz, hipMemcpyDeviceToHost, c->stream));
    CKL(hipStreamSynchronize(c->stream)); CKL(hipGetLastError());
    const int32_t *cnt = a_cnt.at(ho), *roff = a_roff.at(ho);
    const TdRec *first = a_rec.at(ho);
    const size_t n_rec = (size_t)roff[nq];
    std::vector<TdRec> rest;                                           // (only after a call with a max_match above the default)
    if (n_rec > n_first) { rest.resize(n_rec - n_first); CKL(hipMemcpy(rest.data(), a_rec.at(dout) + n_first, sizeof(TdRec)*rest.size(), hipMemcpyDeviceToHost)); }
    a_cnt.get(ho, p->match_cnt);
    int over = -1;
    for (size_t q = 0; q < nq; q++) {
        const size_t n = (size_t)cnt[q];
        if (n > mm) { if (over < 0) over = (int)q; continue; }         // that query's list stays as it was
        for (size_t j = 0; j < n; j++) {
            const size_t at = (size_t)roff[q] + j; const TdRec &r = at < n_first ? first[at] : rest[at - n_first];
            p->match_idx[q*mm + j] = r.idx; p->match_dist[q*mm + j] = r.dist; p->match_score[q*mm + j] = r.score;
        }
    }
    a_ks.get(ho, p->kf_score); a_ko.get(ho, p->kf_nobj);
    const int32_t nc = *a_nc.at(ho);
    *p->n_cand = nc; std::copy_n(a_cand.at(ho), nc, p->cand);
    if (over >= 0) {
        c->err = "tsloop_detect_loop: query " + std::to_string(over) + " has " + std::to_string(cnt[over]) + " matches, more than max_match = " + std::to_string(p->max_match) +
                 " (match_cnt, kf_score, kf_nobj, n_cand and cand are complete; the lists of such queries are not written)";
        return TSLOOP_ERR_ARG;
    }
    return TSLOOP_OK;
}

void tsloop_default_options_loop(tsloop_options *o) {
    tsloop_default_options_sim3(o);
    o->huber_delta = 0.0; o->thresh_outlier = 0.0;            // no loss function (nullptr, optimizer.cc:818,856), no inlier test
}

int tsloop_optimize_loop(void *ctx, tsloop_graph_problem *p, const tsloop_options *o, tsloop_report *r) {
    LCtx *c = (LCtx *)ctx;
    if (!c || !p || !o || !r || p->n_kf <= 0 || p->n_edge < 0 || !p->pose || !p->fixed || (p->n_edge > 0 && (!p->edge_i || !p->edge_j || !p->meas))) return TSLOOP_ERR_ARG;
    for (int e = 0; e < p->n_edge; e++)
        if (p->edge_i[e] < 0 || p->edge_i[e] >= p->n_kf || p->edge_j[e] < 0 || p->edge_j[e] >= p->n_kf || p->edge_i[e] == p->edge_j[e]) { c->err = "bad edge index"; return TSLOOP_ERR_ARG; }
    for (int k = 0; k < p->n_kf; k++) if (!(p->pose[8*k + 7] > 0.0)) { c->err = "scale must be positive"; return TSLOOP_ERR_ARG; }
    hipSetDevice(c->device);
    const auto t0 = std::chrono::steady_clock::now();
    memset(r, 0, sizeof(*r));
    const int N = p->n_kf, E = p->n_edge;
    // ---- host plan: compressed free keyframes, incidence lists, keyframe pairs
    std::vector<int> fidx(N), free_kf; int nf = 0;
    for (int k = 0; k < N; k++) { fidx[k] = p->fixed[k] ? -1 : nf++; if (!p->fixed[k]) free_kf.push_back(k); }
    if (nf == 0 || E == 0) { r->termination = 5; return TSLOOP_ERR_NUMERIC; }
    std::vector<int> kf_off(nf + 1, 0), kf_inc;
    for (int e = 0; e < E; e++) { if (fidx[p->edge_i[e]] >= 0) kf_off[fidx[p->edge_i[e]] + 1]++; if (fidx[p->edge_j[e]] >= 0) kf_off[fidx[p->edge_j[e]] + 1]++; }
    for (int k = 0; k < nf; k++) kf_off[k + 1] += kf_off[k];
    kf_inc.resize(kf_off[nf]);
    { std::vector<int> cur(kf_off.begin(), kf_off.end() - 1);
      for (int e = 0; e < E; e++) { const int fa = fidx[p->edge_i[e]], fb = fidx[p->edge_j[e]];
          if (fa >= 0) kf_inc[cur[fa]++] = e << 1; if (fb >= 0) kf_inc[cur[fb]++] = (e << 1) | 1; } }
    std::map<std::pair<int,int>, std::vector<int>> pm;              // (a > b) -> edges (edge << 1 | side of a)
    for (int e = 0; e < E; e++) { const int fa = fidx[p->edge_i[e]], fb = fidx[p->edge_j[e]];
        if (fa < 0 || fb < 0) continue;
        if (fa > fb) pm[{fa, fb}].push_back(e << 1); else pm[{fb, fa}].push_back((e << 1) | 1); }
    std::vector<int> pair_a, pair_b, pair_off(1, 0), pair_e;
    for (auto &kv : pm) { pair_a.push_back(kv.first.first); pair_b.push_back(kv.first.second); for (int v : kv.second) pair_e.push_back(v); pair_off.push_back((int)pair_e.size()); }
    const int npair = (int)pair_a.size(), n = 7*nf, n6 = (n + 5)/6*6, nb6 = n6/6;
    // ---- device buffers (one allocation)
    // in: [x0 | x1 | fidx | free | ei | ej | meas | kf_off | kf_inc | pair_a | pair_b | pair_off | pair_e | solver fidx | nfree | LmState]
    // scratch: [r | J1 | J2 | cost | ccost | q | sc | part | g | dp | Sy | LD | dbg | S]   (the lists that can be empty are taken one entry longer)
    const size_t NK = (size_t)N, NE = (size_t)E, NF = (size_t)nf, NP = (size_t)npair, N6 = (size_t)n6;
    Layout L(256);
    const auto a_x0 = L.take<double>(8*NK), a_x1 = L.take<double>(8*NK); const auto a_fidx = L.take<int>(NK), a_free = L.take<int>(NF), a_ei = L.take<int>(NE), a_ej = L.take<int>(NE);
    const auto a_meas = L.take<double>(8*NE); const auto a_kfoff = L.take<int>(NF + 1), a_kfinc = L.take<int>(kf_inc.size() + 1), a_pa = L.take<int>(NP + 1), a_pb = L.take<int>(NP + 1),
               a_poff = L.take<int>(NP + 1), a_pe = L.take<int>(pair_e.size() + 1), a_sfidx = L.take<int>((size_t)nb6), a_nfree = L.take<int>(1); const auto a_st = L.take<LmState>(1);
    const size_t in_end = L.mark();
    const auto a_r = L.take<double>(7*NE), a_J1 = L.take<double>(49*NE), a_J2 = L.take<double>(49*NE), a_ce = L.take<double>(NE), a_cce = L.take<double>(NE), a_qe = L.take<double>(NE),
               a_sc = L.take<double>(N6), a_part = L.take<double>(4*NF), a_g = L.take<double>(N6), a_dp = L.take<double>(N6), a_Sy = L.take<double>(N6),
               a_LD = L.take<double>((size_t)std::max(n6, 32*nb6)); const auto a_dbg = L.take<long long>(64); const auto a_S = L.take<double>((N6 + 1)*N6);
    CKL(c->h_stage.grow(in_end)); CKL(c->d_buf.grow(L.mark()));
    void *h = c->h_stage.as(), *d = c->d_buf.as();
    a_x0.put(h, p->pose); a_x1.put(h, p->pose); a_fidx.put(h, fidx.data()); a_free.put(h, free_kf.data());
    a_ei.put(h, p->edge_i); a_ej.put(h, p->edge_j); a_meas.put(h, p->meas); a_kfoff.put(h, kf_off.data()); a_poff.put(h, pair_off.data());
    std::copy(kf_inc.begin(), kf_inc.end(), a_kfinc.at(h)); std::copy(pair_a.begin(), pair_a.end(), a_pa.at(h)); std::copy(pair_b.begin(), pair_b.end(), a_pb.at(h));
    std::copy(pair_e.begin(), pair_e.end(), a_pe.at(h));
    { int *sf = a_sfidx.at(h); for (int k = 0; k < nb6; k++) sf[k] = k; *a_nfree.at(h) = nb6; }
    LmState st0; memset(&st0, 0, sizeof(st0));
    st0.first = 1; st0.need_lin = 1; st0.max_it = o->max_it; st0.radius = o->initial_radius; st0.decrease_factor = 2.0;
    a_st.put(h, &st0);
    CKL(hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, c->stream));
    PgDev P; memset(&P, 0, sizeof(P));
    P.n_kf = N; P.n_edge = E; P.nf = nf; P.n = n; P.n6 = n6; P.npair = npair;
    P.x[0] = a_x0.at(d); P.x[1] = a_x1.at(d); P.fidx_kf = a_fidx.at(d); P.free_kf = a_free.at(d); P.ei = a_ei.at(d); P.ej = a_ej.at(d); P.meas = a_meas.at(d);
    P.r = a_r.at(d); P.J1 = a_J1.at(d); P.J2 = a_J2.at(d); P.cost_e = a_ce.at(d); P.ccost_e = a_cce.at(d); P.q_e = a_qe.at(d);
    P.kf_off = a_kfoff.at(d); P.kf_inc = a_kfinc.at(d); P.pair_a = a_pa.at(d); P.pair_b = a_pb.at(d); P.pair_off = a_poff.at(d); P.pair_e = a_pe.at(d);
    P.sc = a_sc.at(d); P.part = a_part.at(d);
    Work &W = P.W; W.N = n6; W.n_kf = nb6; W.S = a_S.at(d); W.ldS = n6; W.Sy = a_Sy.at(d); W.g = a_g.at(d); W.dp = a_dp.at(d);
    W.LDbuf = a_LD.at(d); W.fidx = a_sfidx.at(d); W.nfree = a_nfree.at(d); W.dbg = a_dbg.at(d); W.st = a_st.at(d);
    // ---- solver selection as in the BA library
    const size_t lds_small = solve_lds_doubles(n6)*sizeof(double);
    const bool use_lds = lds_solver_fits(n6);
    const int lds_diag = (int)(solve_diag_lds_doubles()*sizeof(double)), lds_panel = (CH_NB + 64)*(CH_NB + 1)*(int)sizeof(double), lds_upd = 2*64*(CH_NB + 1)*(int)sizeof(double),
              lds_bs = (CH_NB*(CH_NB + 1) + 2*CH_NB + 8*CH_NB)*(int)sizeof(double);
    if (use_lds) CKL(hipFuncSetAttribute((const void *)k_solve_t<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_small));
    else {
        CKL(hipFuncSetAttribute((const void *)k_solve_t<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_diag));
        CKL(hipFuncSetAttribute((const void *)k_chol_panel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_panel));
        CKL(hipFuncSetAttribute((const void *)k_chol_update, hipFuncAttributeMaxDynamicSharedMemorySize, lds_upd));
        CKL(hipFuncSetAttribute((const void *)k_chol_backsub, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bs));
    }
    auto solve = [&]() {
        if (use_lds) { hipLaunchKernelGGL(k_solve_t<false>, dim3(1), dim3(SOLVE_THREADS), (int)lds_small, c->stream, W, 0); return; }
        const int bw = n6;                                             // dense: every row below a block can be non-zero
        hipLaunchKernelGGL(k_chol_rhs, dim3((n6 + 255)/256), dim3(256), 0, c->stream, W);
        for (int j0 = 0; j0 < n6; j0 += CH_NB) {
            hipLaunchKernelGGL(k_solve_t<true>, dim3(1), dim3(SOLVE_THREADS), lds_diag, c->stream, W, j0);
            const int wr = std::max(0, std::min(bw, n6 - (j0 + 6)));
            hipLaunchKernelGGL(k_chol_panel, dim3(wr/64 + 1), dim3(CH_T), lds_panel, c->stream, W, j0, bw);
            const int nt = (wr + 1 + 63)/64;
            if (wr > 0) hipLaunchKernelGGL(k_chol_update, dim3(nt*(nt + 1)/2), dim3(CH_T), lds_upd, c->stream, W, j0, bw);
        }
        hipLaunchKernelGGL(k_chol_backsub, dim3(1), dim3(1024), lds_bs, c->stream, W, bw);
    };
    // ---- LM: max_it rounds + one to close the last accepted step (gradient test, iteration limit)
    for (int it = 0; it <= o->max_it; it++) {
        hipLaunchKernelGGL(k_pg_linearize, dim3((E + 63)/64), dim3(64), 0, c->stream, P);
        CKL(hipMemsetAsync(W.S, 0, sizeof(double)*(size_t)n6*n6, c->stream));
        hipLaunchKernelGGL(k_pg_assemble, dim3(nf + npair + 1), dim3(64), 0, c->stream, P, *o);
        hipLaunchKernelGGL(k_pg_pre, dim3(1), dim3(1024), 0, c->stream, P, *o);
        if (it == o->max_it) break;
        solve();
        hipLaunchKernelGGL(k_pg_candidate, dim3((nf + 255)/256), dim3(256), 0, c->stream, P);
        hipLaunchKernelGGL(k_pg_trial, dim3((E + 63)/64), dim3(64), 0, c->stream, P);
        hipLaunchKernelGGL(k_pg_decide, dim3(1), dim3(1024), 0, c->stream, P, *o);
    }
    LmState st;
    CKL(hipMemcpyAsync(a_st.at(h), a_st.at(d), a_st.bytes(), hipMemcpyDeviceToHost, c->stream));
    CKL(hipStreamSynchronize(c->stream)); CKL(hipGetLastError());
    a_st.get(h, &st);
    CKL(hipMemcpy(p->pose, st.cur ? P.x[1] : P.x[0], a_x0.bytes(), hipMemcpyDeviceToHost));
    r->iters = st.it; r->accepted = st.accepted; r->termination = st.term; r->cost0 = st.cost0; r->cost1 = st.x_cost;
    r->t_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st.term == 5 ? TSLOOP_ERR_NUMERIC : TSLOOP_OK;
}

}  // extern "C"
