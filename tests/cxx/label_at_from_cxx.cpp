// TEST INFRASTRUCTURE: the labels at a frame's text detection centres (tsba_text_label_at) driven from C++ through adapter/tsba_text_labels.hpp
// (labels_at_centres) over a mock centre type of its own with the shape of TextSLAM's Vec2.
//
//   label_at_from_cxx <dump.bin> <centres.bin> <out.bin>
//     dump.bin: a flat pose problem (textslam_amd.abi.write_dump); centres.bin: [n][2] doubles, the detection centres (x.5 values, one outside the image);
//     1. tsba_pose_optim on the problem (as optimizer::PoseOptim: the context keeps the state of the solve);
//     2. labels_at_centres(ctx, 0, centres, labels) -- and the several-keyframes overload on the same list twice, which must give the same labels;
//     3. writes the optimised pose [7] (doubles) and the labels [n] (floats) to out.bin.
//   Prints "label at from C++: ok" and exits 0, 3 without a HIP device, anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "dump_io.hpp"
#include "tsba_text_labels.hpp"

namespace mockl { struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } }; }
using mockl::Vec2;

static std::string L(const char *base, int l) { char b[64]; snprintf(b, sizeof b, "%s_%d", base, l); return b; }

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s dump.bin centres.bin out.bin\n", argv[0]); return 2; }
    Dump d; if (!read_dump(argv[1], d)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<Vec2> centres;
    { FILE *f = fopen(argv[2], "rb"); if (!f) { perror(argv[2]); return 2; }
      Vec2 c; while (fread(c.v, sizeof(double), 2, f) == 2) centres.push_back(c);
      fclose(f); }
    // ---- the flat problem, straight from the dump (copies of what the solve writes)
    tsba_problem p; memset(&p, 0, sizeof p);
    p.n_kf = (int32_t)(CNT(d, "pose")/7); p.n_pt = (int32_t)CNT(d, "rho"); p.n_text = (int32_t)(CNT(d, "theta")/3); p.n_levels = I32(d, "n_levels")[0];
    for (int k = 0; k < 4; k++) p.K[k] = F64(d, "K")[k];
    std::vector<double> pose(F64(d, "pose"), F64(d, "pose") + CNT(d, "pose")), rho(p.n_pt ? F64(d, "rho") : nullptr, p.n_pt ? F64(d, "rho") + p.n_pt : nullptr),
        theta(F64(d, "theta"), F64(d, "theta") + CNT(d, "theta"));
    std::vector<uint8_t> sgood(CNT(d, "sgood") ? U8(d, "sgood") : nullptr, CNT(d, "sgood") ? U8(d, "sgood") + CNT(d, "sgood") : nullptr),
        tgood(U8(d, "tobs_good"), U8(d, "tobs_good") + CNT(d, "tobs_good")), tfgood(U8(d, "tfgood"), U8(d, "tfgood") + CNT(d, "tfgood"));
    p.pose = pose.data(); p.rho = rho.data(); p.theta = theta.data(); p.kf_initial = U8(d, "kf_initial");
    p.pt_ray = F64(d, "pt_ray"); p.pt_host = I32(d, "pt_host"); p.pt_host_Trw = F64(d, "pt_host_Trw");
    p.text_host = I32(d, "text_host"); p.text_host_Twr = F64(d, "text_host_Twr"); p.text_box_ray = F64(d, "text_box_ray");
    p.n_sgood = (int32_t)sgood.size(); p.sgood = sgood.data();
    p.n_tobs = (int32_t)CNT(d, "tobs_kf"); p.tobs_kf = I32(d, "tobs_kf"); p.tobs_text = I32(d, "tobs_text"); p.tobs_good = tgood.data();
    p.tobs_fgood_off = I32(d, "tobs_fgood_off"); p.tfgood = tfgood.data();
    std::vector<std::vector<const uint8_t *> > planes((size_t)p.n_levels);
    for (int l = 0; l < p.n_levels; l++) {
        p.n_sobs[l] = (int32_t)CNT(d, L("sobs_kf", l)); p.sobs_kf[l] = I32(d, L("sobs_kf", l)); p.sobs_pt[l] = I32(d, L("sobs_pt", l));
        p.sobs_flag[l] = I32(d, L("sobs_flag", l)); p.sobs_uv0[l] = F64(d, L("sobs_uv0", l));
        p.n_tfeat[l] = (int32_t)CNT(d, L("tfeat_raw", l)); p.tfeat_off[l] = I32(d, L("tfeat_off", l)); p.tfeat_raw[l] = I32(d, L("tfeat_raw", l));
        p.tfeat_uv[l] = F64(d, L("tfeat_uv", l)); p.tfeat_ref[l] = F64(d, L("tfeat_ref", l));
        const int32_t *wh = I32(d, L("img_wh", l)); const uint8_t *im = U8(d, L("img", l));
        if (!wh || !im) continue;
        p.img_w[l] = wh[0]; p.img_h[l] = wh[1];
        for (int k = 0; k < p.n_kf; k++) planes[(size_t)l].push_back(im + (size_t)k*wh[0]*wh[1]);
        p.img[l] = planes[(size_t)l].data();
    }
    if (p.n_kf != 1 || p.n_tobs == 0) { fprintf(stderr, "not a pose problem with text\n"); return 2; }

    void *ctx = nullptr; const int r0 = tsba_create(&ctx, 0);
    if (r0 == TSBA_ERR_DEVICE) { printf("no HIP device\n"); return 3; }
    if (r0) return 1;
    std::vector<float> early;
    if (tsba_adapter::labels_at_centres(ctx, 0, centres, early) != TSBA_ERR_STATE || !early.empty()) { fprintf(stderr, "labels before any solve: no TSBA_ERR_STATE\n"); return 1; }
    tsba_options o; tsba_report rep; tsba_default_options_pose(&o);
    int rc = tsba_pose_optim(ctx, &p, &o, &rep);
    if (rc != TSBA_OK && rc != TSBA_ERR_NUMERIC) { fprintf(stderr, "tsba_pose_optim: %d (%s)\n", rc, tsba_last_error(ctx)); return 1; }
    std::vector<float> labels;
    rc = tsba_adapter::labels_at_centres(ctx, 0, centres, labels);
    if (rc != TSBA_OK || labels.size() != centres.size()) { fprintf(stderr, "labels_at_centres: %d (%s)\n", rc, tsba_last_error(ctx)); return 1; }
    std::vector<std::vector<float> > twice;
    rc = tsba_adapter::labels_at_centres(ctx, std::vector<int>(2, 0), std::vector<const std::vector<Vec2> *>(2, &centres), twice);
    if (rc != TSBA_OK || twice.size() != 2 || twice[0] != labels || twice[1] != labels) { fprintf(stderr, "the several-keyframes overload differs\n"); return 1; }
    std::vector<Vec2> none; std::vector<float> empty(3, 7.0f);
    if (tsba_adapter::labels_at_centres(ctx, 0, none, empty) != TSBA_OK || !empty.empty()) { fprintf(stderr, "no centres: not an empty result\n"); return 1; }
    tsba_destroy(ctx);
    FILE *f = fopen(argv[3], "wb"); if (!f) { perror(argv[3]); return 2; }
    fwrite(pose.data(), sizeof(double), 7, f); fwrite(labels.data(), sizeof(float), labels.size(), f);
    fclose(f);
    printf("label at from C++: ok (%zu centres)\n", centres.size());
    return 0;
}
