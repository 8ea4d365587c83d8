// textslam_traits.hpp -- the Traits of adapter/tsba_gather.hpp over the REAL TextSLAM types.  Lives in the TextSLAM tree (it needs
// TextSLAM's headers, Eigen and OpenCV: not compiled by this repository -- the same templates are compiled and run here against
// tests/cxx/mock_textslam.hpp, whose Traits has exactly these members).
#ifndef TEXTSLAM_TRAITS_HPP
#define TEXTSLAM_TRAITS_HPP
#include <Eigen/Geometry>
#include <opencv2/core/core.hpp>
#include <setting.h>
#include <frame.h>
#include <keyframe.h>
#include <mapPts.h>
#include <mapText.h>
#include <map.h>
#include <Random.h>

namespace tsba_adapter {

struct TextSlamTraits {
    typedef TextSLAM::map Map; typedef TextSLAM::keyframe KeyFrame; typedef TextSLAM::frame Frame;
    typedef TextSLAM::mapPts MapPt; typedef TextSLAM::mapText MapText;
    static TextSLAM::TextStatus text_good() { return TextSLAM::TEXTGOOD; }
    // optimizer.cc:84-90 / :264-271: Eigen::Quaterniond q(Rcw); q = q.normalized();  pose = (w, x, y, z, t)
    static void quat_of(const TextSLAM::Mat33 &R, double q[4]) {
        Eigen::Quaterniond e(R); e = e.normalized();
        q[0] = e.w(); q[1] = e.x(); q[2] = e.y(); q[3] = e.z();
    }
    // optimizer.cc:292-312: normalise the quaternion, build Tcw, SetPose
    template <class PoseHolder> static void set_pose(PoseHolder &kf, const double pose[7]) {
        Eigen::Quaterniond qcw; qcw.w() = pose[0]; qcw.x() = pose[1]; qcw.y() = pose[2]; qcw.z() = pose[3];
        qcw = qcw.normalized();
        TextSLAM::Mat33 Rcw(qcw);
        TextSLAM::Mat44 Tcw; Tcw.setIdentity();
        Tcw.block<3, 3>(0, 0) = Rcw; Tcw.block<3, 1>(0, 3) = TextSLAM::Mat31(pose[4], pose[5], pose[6]);
        kf.SetPose(Tcw);
    }
    // optimizer.cc:321-325
    static void set_theta(MapText &obj, const double th[3]) { TextSLAM::Mat31 N(th[0], th[1], th[2]); obj.RefKF->SetN(N, obj.GetNidx()); }
    // ---- loop closing (adapter/tsloop_gather.hpp): the reference's own Sim3_loop (setting.h:129-171) does the algebra
    typedef TextSLAM::Sim3_loop Sim3;
    static Sim3 sim_make(const double q[4], const double t[3], double s) {
        Eigen::Quaterniond e(q[0], q[1], q[2], q[3]); e = e.normalized();
        return Sim3(e, Eigen::Vector3d(t[0], t[1], t[2]), s);
    }
    static Sim3 sim_of_pose(const TextSLAM::Mat33 &R, const TextSLAM::Mat31 &t, double s) { return Sim3(R, t, s); }     // optimizer.cc:794-796
    static void sim_get(const Sim3 &S, bool normalise, double out[8]) {
        Eigen::Quaterniond e = S.r; if (normalise) e = e.normalized();
        out[0] = e.w(); out[1] = e.x(); out[2] = e.y(); out[3] = e.z(); out[4] = S.t(0); out[5] = S.t(1); out[6] = S.t(2); out[7] = S.s;
    }
    // optimizer.cc:887-906: q normalised, T = [R(q) | t / s], SetPose(T)
    static void set_pose_sim(KeyFrame &kf, const double pose[8]) {
        const double p7[7] = { pose[0], pose[1], pose[2], pose[3], pose[4]/pose[7], pose[5]/pose[7], pose[6]/pose[7] };
        set_pose(kf, p7);
    }
    // ---- loop fusion's window searches (adapter/tsorb_loop_fuse.hpp; `using tsorb_adapter::FUSE_*` values 0 / 1 / 2 = searched / negative depth / outside the image)
    static int rows(const cv::Mat &m) { return m.rows; }
    static const uint8_t *row(const cv::Mat &m, int i) { return m.ptr<uint8_t>(i); }
    // loopClosing.cc:1172-1181 and :1196-1211, SearchAndFuse_Scene's own expressions: Tcw = [R | t / s], Tcr, Pc, the depth test, mK * Pc, IsInImage -- all in doubles
    static int fuse_project(KeyFrame *kf, const Sim3 &S, MapPt *pt, double &u, double &v) {
        using namespace TextSLAM;
        Mat44 T_cw = Mat44::Identity();                                        // [R | t / s]
        T_cw.block<3, 3>(0, 0) = Mat33(S.r);
        Mat31 t = S.t; t /= S.s; T_cw.block<3, 1>(0, 3) = t;
        const Mat44 T_cr = T_cw * pt->RefKF->mTcw.inverse();
        const Mat31 p_r = pt->GetRaydir()/pt->GetInverD();
        const Mat31 p_c = T_cr.block<3, 3>(0, 0) * p_r + T_cr.block<3, 1>(0, 3);
        if (p_c(2, 0) < 0.0) return 1;
        const Mat31 h = kf->mK * p_c;
        u = h(0)/h(2); v = h(1)/h(2);
        return kf->IsInImage(u, v) ? 0 : 2;
    }
    // loopClosing.cc:1422-1432, MatchMore's own expressions (products in its order: (R * invrho) * ray, K * (R p + t))
    static void more_project(KeyFrame *kf1, KeyFrame *kf2, const Sim3 &g, MapPt *pt, double &u, double &v) {
        using namespace TextSLAM;
        const Mat31 ray = pt->GetRaydir(); const double inv_rho = 1.0/pt->GetInverD();
        const Mat44 T = kf2->mTcw * pt->RefKF->mTwc;
        const Eigen::Quaterniond q = g.r; const Mat33 R(q);
        const Mat31 p2 = T.block<3, 3>(0, 0) * inv_rho * ray + T.block<3, 1>(0, 3);
        const Mat31 h = kf1->mK * (R * p2 + g.t);
        u = h(0)/h(2); v = h(1)/h(2);
    }
    // Sim3Solver's index draws (adapter/tsloop_sim3_ransac.hpp): the reference's own generator, Sim3Solver.cc:81
    static int random_int(int lo, int hi) { return DUtils::Random::RandomInt(lo, hi); }
    // the planes of new text detections (adapter/tsorb_text_theta.hpp): tool.cc:1375 / initializer.cc:130; tracking.cc:1667 / initializer.cc:1013, the reference's own expression
    static void seed_rand_once() { DUtils::Random::SeedRandOnce(0); }
    static void tcr_of(const TextSLAM::Mat44 &Tcw, const TextSLAM::Mat44 &Trw, double out[12]) {
        const TextSLAM::Mat44 Tcr = Tcw * Trw.inverse();
        for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) out[4*r + c] = Tcr(r, c);
    }
    static TextSLAM::Mat31 vec3(double a, double b, double c) { return TextSLAM::Mat31(a, b, c); }
    // a new keyframe's scene points and the initializer's search (adapter/tsorb_new_points.hpp) use row() and vec3() above: nothing else is needed
    // nume_BAText.h:25: the cost functors index cv::Mat::data directly, i.e. continuous CV_8UC1 with step == cols
    static const uint8_t *img(const cv::Mat &im) { CV_Assert(im.type() == CV_8UC1 && im.isContinuous()); return im.data; }
    static int img_w(const cv::Mat &im) { return im.cols; }
    static int img_h(const cv::Mat &im) { return im.rows; }
};

}  // namespace tsba_adapter
#endif
