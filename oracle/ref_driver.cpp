// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.
//
// C entry points over TextSLAM's own cost functors, compiled from the reference tree's include/ directory against the stand-in
// headers of oracle/ref_shims/ (oracle/Makefile, target _ref/libtsref.so; nothing of that tree or of this library is committed).
// Each entry point builds the functor with the constructor arguments optimizer.cc gives it and calls its operator() once per
// block: plain doubles for the residuals, and for the templated (auto_*) functors once more on Jets for the Jacobian with
// respect to the ambient parameter blocks, concatenated in the functor's parameter order.
// All matrices cross this boundary row-major; K is 3x3; a pose matrix is 4x4.
#include <stdint.h>
#include <vector>
#include "auto_BAScene.h"
#include "auto_BASceneNW.h"
#include "auto_IniBAScene.h"
#include "auto_PoseOptimScene.h"
#include "auto_RhoScene.h"
#include "auto_sim.h"
#include "auto_siminv.h"
#include "nume_BAText.h"
#include "nume_IniBAText.h"
#include "nume_PoseOptimText.h"
#include "nume_thetaText.h"
#include "numer_loop_ver2.h"

namespace {

typedef Eigen::Matrix<double, 2, 1> V2;
typedef Eigen::Matrix<double, 3, 1> V3;
typedef Eigen::Matrix<double, 3, 3> M3;
typedef Eigen::Matrix<double, 4, 4> M4;

M3 mat3(const double *k) { M3 m; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m(i, j) = k[3*i + j]; return m; }
M4 mat4(const double *t) { M4 m; for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) m(i, j) = t[4*i + j]; return m; }

// the parameter blocks of one residual block as Jets over all N ambient coordinates: block b starts at column off[b]
template <int N> void seed(const double *x, int len, int off, ceres::Jet<double, N> *out) {
    for (int i = 0; i < len; i++) out[i] = ceres::Jet<double, N>(x[i], off + i);
}
template <int N, int NR> void unpack(const ceres::Jet<double, N> *r, double *jac) {
    for (int k = 0; k < NR; k++) for (int c = 0; c < N; c++) jac[k*N + c] = r[k].v[c];
}

std::vector<V3> rays_of(const double *r) { std::vector<V3> v(8); for (int k = 0; k < 8; k++) v[k] = V3(r[3*k], r[3*k + 1], r[3*k + 2]); return v; }
std::vector<double> ref_of(const double *r) { return std::vector<double>(r, r + 8); }

}  // namespace

extern "C" {

int tsref_abi(void) { return 1; }

// auto_BAScene (nw == 0) / auto_BASceneNW (nw == 1); jac [n][2][15] over (qcw 4 | tcw 3 | qrw 4 | trw 3 | rho 1), may be NULL
void tsref_ba_scene(int n, int nw, const double *obv, const double *ray, const double *K, double wx, double wy, const double *qcw, const double *tcw,
                    const double *qrw, const double *trw, const double *rho, double *res, double *jac) {
    typedef ceres::Jet<double, 15> J;
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        const V2 o(obv[2*i], obv[2*i + 1]); const V3 r(ray[3*i], ray[3*i + 1], ray[3*i + 2]);
        J a[4], b[3], c[4], d[3], e[1], rj[2];
        seed<15>(qcw + 4*i, 4, 0, a); seed<15>(tcw + 3*i, 3, 4, b); seed<15>(qrw + 4*i, 4, 7, c); seed<15>(trw + 3*i, 3, 11, d); seed<15>(rho + i, 1, 14, e);
        if (nw) {
            auto_BASceneNW f(o, r, Km);
            f(qcw + 4*i, tcw + 3*i, qrw + 4*i, trw + 3*i, rho + i, res + 2*i);
            if (jac) f(a, b, c, d, e, rj);
        } else {
            auto_BAScene f(o, r, Km, wx, wy);
            f(qcw + 4*i, tcw + 3*i, qrw + 4*i, trw + 3*i, rho + i, res + 2*i);
            if (jac) f(a, b, c, d, e, rj);
        }
        if (jac) unpack<15, 2>(rj, jac + 30*i);
    }
}

// auto_PoseOptimScene; rayrho = (mx, my, rho), Trw [n][16]; jac [n][2][7] over (q 4 | t 3)
void tsref_pose_scene(int n, const double *obv, const double *rayrho, const double *Trw, const double *K, double wx, double wy,
                      const double *q, const double *t, double *res, double *jac) {
    typedef ceres::Jet<double, 7> J;
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        auto_PoseOptimScene f(V2(obv[2*i], obv[2*i + 1]), V3(rayrho[3*i], rayrho[3*i + 1], rayrho[3*i + 2]), mat4(Trw + 16*i), Km, wx, wy);
        f(q + 4*i, t + 3*i, res + 2*i);
        if (jac) { J a[4], b[3], rj[2]; seed<7>(q + 4*i, 4, 0, a); seed<7>(t + 3*i, 3, 4, b); f(a, b, rj); unpack<7, 2>(rj, jac + 14*i); }
    }
}

// auto_IniBAScene; jac [n][2][8] over (q 4 | t 3 | rho 1)
void tsref_ini_scene(int n, const double *obv, const double *ray, const double *K, const double *q, const double *t, const double *rho, double *res, double *jac) {
    typedef ceres::Jet<double, 8> J;
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        auto_IniBAScene f(V2(obv[2*i], obv[2*i + 1]), V3(ray[3*i], ray[3*i + 1], ray[3*i + 2]), Km);
        f(q + 4*i, t + 3*i, rho + i, res + 2*i);
        if (jac) { J a[4], b[3], c[1], rj[2]; seed<8>(q + 4*i, 4, 0, a); seed<8>(t + 3*i, 3, 4, b); seed<8>(rho + i, 1, 7, c); f(a, b, c, rj); unpack<8, 2>(rj, jac + 16*i); }
    }
}

// auto_RhoScene; Tcr [n][16]; jac [n][2][1] over rho
void tsref_rho_scene(int n, const double *obv, const double *ray, const double *Tcr, const double *K, const double *rho, double *res, double *jac) {
    typedef ceres::Jet<double, 1> J;
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        auto_RhoScene f(V2(obv[2*i], obv[2*i + 1]), V3(ray[3*i], ray[3*i + 1], ray[3*i + 2]), mat4(Tcr + 16*i), Km);
        f(rho + i, res + 2*i);
        if (jac) { J a[1], rj[2]; seed<1>(rho + i, 1, 0, a); f(a, rj); unpack<1, 2>(rj, jac + 2*i); }
    }
}

// the four text functors: 8 taps per block; imgs [n] image pointers (w x h, uint8), rays [n][8][3], ref [n][8], res [n][8]
void tsref_ba_text(int n, const uint8_t *const *imgs, int w, int h, const double *rays, const double *ref, const double *mu, const double *sigma,
                   const double *K, double wT, const double *qcw, const double *tcw, const double *qrw, const double *trw, const double *theta, double *res) {
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        nume_BAText f(cv::Mat(h, w, (unsigned char *)imgs[i]), rays_of(rays + 24*i), ref_of(ref + 8*i), mu[i], sigma[i], Km, wT);
        f(qcw + 4*i, tcw + 3*i, qrw + 4*i, trw + 3*i, theta + 3*i, res + 8*i);
    }
}
void tsref_pose_text(int n, const uint8_t *const *imgs, int w, int h, const double *Twr, const double *theta, const double *rays, const double *ref,
                     const double *mu, const double *sigma, const double *K, double wT, const double *q, const double *t, double *res) {
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        nume_PoseOptimText f(cv::Mat(h, w, (unsigned char *)imgs[i]), mat4(Twr + 16*i), V3(theta[3*i], theta[3*i + 1], theta[3*i + 2]), rays_of(rays + 24*i),
                             ref_of(ref + 8*i), mu[i], sigma[i], Km, wT);
        f(q + 4*i, t + 3*i, res + 8*i);
    }
}
void tsref_ini_text(int n, const uint8_t *const *imgs, int w, int h, const double *rays, const double *ref, const double *mu, const double *sigma,
                    const double *K, const double *q, const double *t, const double *theta, double *res) {
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        nume_IniBAText f(cv::Mat(h, w, (unsigned char *)imgs[i]), rays_of(rays + 24*i), ref_of(ref + 8*i), mu[i], sigma[i], Km);
        f(q + 4*i, t + 3*i, theta + 3*i, res + 8*i);
    }
}
void tsref_theta_text(int n, const uint8_t *const *imgs, int w, int h, const double *rays, const double *ref, const double *mu, const double *sigma,
                      const double *Tcr, const double *K, const double *theta, double *res) {
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        nume_thetaText f(cv::Mat(h, w, (unsigned char *)imgs[i]), rays_of(rays + 24*i), ref_of(ref + 8*i), mu[i], sigma[i], mat4(Tcr + 16*i), Km);
        f(theta + 3*i, res + 8*i);
    }
}

// auto_sim (inv == 0): P = the point in camera 2, obv = its pixel in image 1; auto_siminv (inv == 1): the other way round.
// One Sim3 x = (q 4 | t 3 | s 1) for all n matches; jac [n][2][8], may be NULL
void tsref_sim(int n, int inv, const double *P, const double *obv, const double *K, const double *x, double *res, double *jac) {
    typedef ceres::Jet<double, 8> J;
    const M3 Km = mat3(K);
    J a[4], b[3], c[1], rj[2];
    seed<8>(x, 4, 0, a); seed<8>(x + 4, 3, 4, b); seed<8>(x + 7, 1, 7, c);
    for (int i = 0; i < n; i++) {
        const V3 p(P[3*i], P[3*i + 1], P[3*i + 2]); const V2 o(obv[2*i], obv[2*i + 1]);
        if (inv) { auto_siminv f(p, o, Km); f(x, x + 4, x + 7, res + 2*i); if (jac) f(a, b, c, rj); }
        else { auto_sim f(p, o, Km); f(x, x + 4, x + 7, res + 2*i); if (jac) f(a, b, c, rj); }
        if (jac) unpack<8, 2>(rj, jac + 16*i);
    }
}

// numer_loop_ver2: meas = S21 (q | t | s) per edge, x1 / x2 the two keyframes' Sim3; res [n][7]
void tsref_loop(int n, const double *meas, const double *x1, const double *x2, double *res) {
    for (int i = 0; i < n; i++) {
        const double *m = meas + 8*i, *a = x1 + 8*i, *b = x2 + 8*i;
        numer_loop_ver2 f(Eigen::Quaterniond(m[0], m[1], m[2], m[3]), Eigen::Vector3d(m[4], m[5], m[6]), m[7]);
        f(a, a + 4, a + 7, b, b + 4, b + 7, res + 7*i);
    }
}

// logSim3 (ModelTool.hpp): q [n][4] as given (not normalised here), t [n][3], s [n]; res [n][7]
void tsref_logsim3(int n, const double *q, const double *t, const double *s, double *res) {
    for (int i = 0; i < n; i++) {
        const Eigen::Matrix<double, 7, 1> r = logSim3(Eigen::Quaterniond(q[4*i], q[4*i + 1], q[4*i + 2], q[4*i + 3]), Eigen::Vector3d(t[3*i], t[3*i + 1], t[3*i + 2]), s[i]);
        for (int k = 0; k < 7; k++) res[7*i + k] = r(k);
    }
}

// TextProj (ModelTool.hpp), both overloads: the point in the target camera p [n][3] and, through K, its pixel uv [n][2]
void tsref_textproj(int n, const double *ray, const double *Tcr, const double *theta, const double *K, double *p, double *uv) {
    const M3 Km = mat3(K);
    for (int i = 0; i < n; i++) {
        const V3 r(ray[3*i], ray[3*i + 1], ray[3*i + 2]), th(theta[3*i], theta[3*i + 1], theta[3*i + 2]); const M4 T = mat4(Tcr + 16*i);
        const V3 P = TextProj(r, T, th); const V2 u = TextProj(r, T, th, Km);
        for (int k = 0; k < 3; k++) p[3*i + k] = P(k);
        uv[2*i] = u(0); uv[2*i + 1] = u(1);
    }
}

}  // extern "C"
