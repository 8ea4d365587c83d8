"""Text paths on images above 640 x 480: the quad's bit mask in row bands (tsraster.h raster_quad_rows; csrc/tsquadstat.h quad_moments and k_label band every
level, and a level of at most 640 x 480 is one band: there is one path) and the judge's association by point tests.  Every test fails with TSBA_ERR_ARG /
TSFRAME_ERR_ARG on a build that caps the text paths at 640 x 480.

Sizes: 648 x 480 (just past the mask: 474-row bands, only level 0 takes more than one), 1280 x 720 (240-row bands; levels 1 and 2 fit one band: both in one
solve), 1920 x 1080 (levels 0 and 1 in several bands: 160- and 320-row bands); box by box also 640 x 480 itself, where plane c's single band is all 480 rows
and so every word of the mask.  Tolerances: those of the 640 x 480 tests (test_gpu_parity, test_gpu_theta_batch,
test_gpu_label_at, test_gpu_text_judge) unchanged -- the arithmetic is the same, only the mask's addressing differs; label images and the judge's bits are exact.
The synthetic problems are synth.camera's; the oracle's results are computed once per size and shared."""
import functools
import os
import sys

import numpy as np
import pytest

from textslam_amd import synth, abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_label_at import _rays_for, _corners, _ranks                          # noqa: E402
from test_gpu_parity import _check_solve                                                     # noqa: E402
from test_gpu_text_judge import _check_against_ref, PASS                                     # noqa: E402

pytestmark = pytest.mark.gpu

MASK_BITS = 9600*32                                          # MS_MASK_WORDS*32 (csrc/tsraster.h)
SIZES = [(648, 480), (1280, 720), (1920, 1080)]
MID = (1280, 720)


def camera_K(w, h):
    """the 640 x 480 GeneralMotion camera scaled to w x h: focal lengths by w / 640, the principal point with the image"""
    fx, fy, cx, cy = synth.K_GENERAL_MOTION
    return np.array([fx*w/640.0, fy*w/640.0, cx*w/640.0, cy*h/480.0])


def band_rows(w):
    return MASK_BITS//w


def is_big(w, h):
    return w*h > MASK_BITS


@functools.lru_cache(maxsize=None)
def tiny_at(w, h):
    with synth.camera(w, h, camera_K(w, h)):
        return synth.tiny()


def clamped_rows(P, level, kf, j):
    """(yMin, yMax) of the clamped bounding box of plane j in keyframe kf, as musigma_core takes them (tool::CalTextinfo: ceil / floor of the corners)"""
    hh = int(P.img[level].shape[1])
    cv = _corners(P, level, kf, j)[:, 1]
    y_max = max([int(np.ceil(v)) for v in cv if v > -1.0] + [-1])
    y_min = min([int(np.floor(v)) for v in cv if v < hh + 1] + [hh + 1])
    return min(max(y_min, 0), hh - 1), max(min(y_max, hh - 1), 0)


@functools.lru_cache(maxsize=None)
def boxes_at(w, h):
    """tiny() at w x h with the box rays of three planes replaced so that, at level 0 of the newest keyframe, plane a projects inside one band, plane b taller than
    one band and fully inside the image, plane c over the whole image with all four corners outside.  Returns (problem, (a, b, c)).  The planes are those the
    newest keyframe observes (three of them, in tiny())."""
    P = tiny_at(w, h).copy()
    kf = P.n_kf - 1
    seen = [int(P.tobs_text[t]) for t in _ranks(P, kf)]
    order = seen + [j for j in range(P.n_text) if j not in seen]
    c, b, a = sorted(order[:3])                              # (a keyframe's quads are painted in plane order: c first, b over it, a last -- all three stay visible)
    B = band_rows(w)
    ha = min(B//4, 40)
    target = {
        a: [(0.40*w, 0.5*h - ha), (0.55*w, 0.5*h - ha + 5), (0.56*w, 0.5*h + ha), (0.39*w, 0.5*h + ha - 4)],
        b: [(0.20*w, 2.5), (0.45*w, 3.5), (0.47*w, h - 2.5), (0.18*w, h - 3.5)],
        c: [(-0.30*w, -0.30*h), (1.30*w, -0.25*h), (1.35*w, 1.30*h), (-0.25*w, 1.20*h)],
    }
    box = np.asarray(P.text_box_ray, np.float64).reshape(-1, 4, 2).copy()
    for j, uv in target.items():
        box[j] = _rays_for(P, 0, kf, j, uv)
    P.text_box_ray = box
    return P.normalise(), (a, b, c)


@functools.lru_cache(maxsize=None)
def boxes_oracle(w, h):
    """the oracle's mu / sigma [level][n_tobs, 2] and label images [level] (newest keyframe) of boxes_at(w, h)"""
    import oracle
    P, _ = boxes_at(w, h)
    o = abi.options_local()
    ms = [oracle.evaluate(P, o, l, jac=False)["musigma"].copy() for l in range(P.n_levels)]
    lab = [oracle.label_image(P, P.n_kf - 1, l) for l in range(P.n_levels)]
    return ms, lab


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


# ------------------------------------------------------------------ mu / sigma and label image, box by box
def check_box_conditions(w, h):
    """What the boxes must be for the device comparison to mean anything, from the oracle and the geometry alone (no device): returns the figures it checked."""
    P, (a, b, c) = boxes_at(w, h)
    ms, _ = boxes_oracle(w, h)
    kf = P.n_kf - 1
    out = []
    for l in range(P.n_levels):
        hh, ww = int(P.img[l].shape[1]), int(P.img[l].shape[2])
        valid = (ms[l][:, 0] != 0.0) | (ms[l][:, 1] != 0.0)               # (n < 2 leaves mu = sigma = 0; the rendered images have no zero pixels)
        for j in (a, b, c):
            obs = np.nonzero((np.asarray(P.tobs_text) == j) & (np.asarray(P.tobs_kf) != P.text_host[j]))[0]      # (a host's view of its own plane has no blocks and no moments)
            assert obs.size > 0 and kf in P.tobs_kf[obs] and valid[obs].all(), (w, h, l, j, ms[l][obs])
        assert P.n_tobs == 14 and int(valid.sum()) >= 10, (w, h, l, int(valid.sum()))
        rows = {j: clamped_rows(P, l, kf, j) for j in (a, b, c)}
        span = {j: rows[j][1] - rows[j][0] + 1 for j in rows}
        if is_big(ww, hh):
            B = band_rows(ww)
            assert span[a] <= B and span[b] > B and span[c] > B, (w, h, l, span, B)
        if l == 0:
            ca, cb, cc = (_corners(P, 0, kf, j) for j in (a, b, c))
            assert (cb[:, 0] > 0).all() and (cb[:, 0] < ww - 1).all() and (cb[:, 1] > 0).all() and (cb[:, 1] < hh - 1).all()
            assert all(u < 0 or u > ww or v < 0 or v > hh for u, v in cc) and cc[:, 0].min() < 0 and cc[:, 0].max() > ww and cc[:, 1].min() < 0 and cc[:, 1].max() > hh
            assert (ca[:, 0] > 0).all() and (ca[:, 0] < ww - 1).all() and (ca[:, 1] > 0).all() and (ca[:, 1] < hh - 1).all()
        out.append((l, ww, hh, int(valid.sum()), span))
    return out


@pytest.mark.parametrize("w,h", [(640, 480)] + SIZES)
def test_musigma_and_label_image_box_by_box(gpu, oracle_lib, w, h):
    P, (a, b, c) = boxes_at(w, h)
    if (w, h) == (640, 480):                                 # the one band of plane c is the whole level: every word of the mask
        assert w*h == MASK_BITS and clamped_rows(P, 0, P.n_kf - 1, c) == (0, h - 1)
    for fig in check_box_conditions(w, h):
        print("%d x %d level %d (%d x %d): %d of 14 observations with moments, rows of (a, b, c) %s" % ((w, h) + fig[:4] + (fig[4],)))
    ms, lab = boxes_oracle(w, h)
    o = abi.options_local()
    kf = P.n_kf - 1
    for l in range(P.n_levels):
        eg = gpu.evaluate(P, o, l, jac=False)
        np.testing.assert_allclose(eg["musigma"], ms[l], rtol=1e-11, atol=1e-10)
        hh, ww = int(P.img[l].shape[1]), int(P.img[l].shape[2])
        img = gpu.TextLabelImage(kf, l, (hh, ww))                       # (the state the evaluation uploaded: P's parameters)
        nbad = int(np.count_nonzero(img != lab[l]))
        print("level %d: %d labelled pixels, %d differ from the oracle" % (l, int((lab[l] >= 0).sum()), nbad))
        assert img.shape == lab[l].shape and nbad == 0, (l, nbad)
        ranks = {int(j): r for r, j in enumerate(P.tobs_text[_ranks(P, kf)])}
        assert all(np.any(lab[l] == ranks[j]) for j in (a, b, c)), (l, ranks)                 # each of the three quads shows in the image
        # the labels at the box centres, without the image
        cen = np.array([np.rint(_corners(P, l, kf, j).mean(0)) for j in range(P.n_text)]).astype(np.int32)
        cen = cen[(cen[:, 0] >= 0) & (cen[:, 0] < ww) & (cen[:, 1] >= 0) & (cen[:, 1] < hh)]
        at = gpu.TextLabelAt(l, kf, cen)
        assert len(cen) >= 3 and np.array_equal(at.astype(np.float32), img[cen[:, 1], cen[:, 0]]), (l, at)


# ------------------------------------------------------------------ solves
@functools.lru_cache(maxsize=None)
def pose_window_at(w, h):
    return synth.window_of(tiny_at(w, h), tiny_at(w, h).n_kf - 1, 1)


@pytest.mark.parametrize("w,h", SIZES)
def test_local_ba(gpu, oracle_lib, w, h):
    G, rep = _check_solve(gpu, oracle_lib, tiny_at(w, h), abi.options_local(), lambda G, o: gpu.LocalBundleAdjustment(G, options=o))
    assert sum(rep["iters"]) > 0 and rep["n_tblock"][0] > 0


@pytest.mark.parametrize("w,h", SIZES)
def test_pose_optim_on_a_window(gpu, oracle_lib, w, h):
    P = pose_window_at(w, h)
    assert P.n_kf == 1 and P.n_tobs > 0
    G, rep = _check_solve(gpu, oracle_lib, P, abi.options_pose(), lambda G, o: gpu.PoseOptim(G, options=o))
    assert sum(rep["iters"]) > 0 and rep["n_tblock"][0] > 0


def test_local_ba_launch_per_step(gpu, oracle_lib):
    """the same window with tsba_debug_options.pass_launches = 2: the stand-alone mu / sigma launch of the generic pass"""
    try:
        gpu.debug_set(pass_launches=2)
        _check_solve(gpu, oracle_lib, tiny_at(*MID), abi.options_local(), lambda G, o: gpu.LocalBundleAdjustment(G, options=o))
    finally:
        gpu.debug_set()


def test_init_ba(gpu, oracle_lib):
    with synth.camera(*MID, camera_K(*MID)):
        P = synth.init_pair(seed=5)
    G, rep = _check_solve(gpu, oracle_lib, P, abi.options_init(), lambda G, o: gpu.InitBA(G, options=o), atol=1e-4, rtol_cost=1e-5)      # (test_init_ba_parity's)
    assert rep["n_passes"] == 4 and P.img[0].shape[1:] == (720, 1280)


def test_landmarker(gpu, oracle_lib):
    with synth.camera(*MID, camera_K(*MID)):
        P = synth.landmark_refine(seed=9)
    G, rep = _check_solve(gpu, oracle_lib, P, abi.options_landmarker(), lambda G, o: gpu.OptimizeLandmarker(G, options=o))
    assert np.array_equal(G.pose, P.pose) and not np.array_equal(G.rho, P.rho)


# ------------------------------------------------------------------ theta solves
def test_theta_single_and_batch(gpu, oracle_lib):
    """tsba_theta_optim and tsba_theta_optim_batch at 1280 x 720.  Bit for bit: a plane in the batch of four against the same plane alone in a batch (what
    test_batch_planes_are_independent_and_deterministic holds at 640 x 480).  The two ENTRY POINTS are different kernels and agree within rounding at any size
    (test_batch_matches_single_calls: 1e-8 / 1e-7; measured here 5e-16 .. 5e-15 on theta): both are held to the oracle and to each other at those tolerances."""
    with synth.camera(*MID, camera_K(*MID)):
        planes = synth.theta_planes(seed=5, n=4)
    o = abi.options_theta()
    work = [P.copy() for P in planes]
    reps, covs = gpu.ThetaOptimMultiFsBatch(work, options=o)
    for i, P in enumerate(planes):
        R, G, B1 = P.copy(), P.copy(), P.copy()
        rc, rep_o, cov_o = oracle_lib.theta_optim(R, o, 0)
        rep_s, cov_s = gpu.ThetaOptimMultiFs(G, text=0, options=o)
        reps1, covs1 = gpu.ThetaOptimMultiFsBatch([B1], options=o)
        print("plane %d: iters %s, |theta batch - single call| %.3e, |batch - oracle| %.3e" % (i, rep_o["iters"], np.abs(work[i].theta - G.theta).max(), np.abs(work[i].theta - R.theta).max()))
        # the batch of four against the plane alone in a batch: bit for bit
        assert work[i].theta.tobytes() == B1.theta.tobytes() and covs[i].tobytes() == covs1[0].tobytes(), i
        assert reps[i]["iters"] == reps1[0]["iters"] and reps[i]["accepted"] == reps1[0]["accepted"] and reps[i]["termination"] == reps1[0]["termination"]
        # both entry points against the oracle, covariance included (test_batch_matches_oracle_per_plane / test_theta_optim_parity_and_covariance)
        for rep, th, cov in ((reps[i], work[i].theta, covs[i]), (rep_s, G.theta, cov_s)):
            assert rep["iters"] == rep_o["iters"] and rep["accepted"] == rep_o["accepted"] and rep["termination"] == rep_o["termination"], (i, rep, rep_o)
            np.testing.assert_allclose(rep["cost0"], rep_o["cost0"], rtol=1e-9)
            np.testing.assert_allclose(rep["cost1"], rep_o["cost1"], rtol=1e-9)
            np.testing.assert_allclose(th, R.theta, rtol=0, atol=1e-8)
            assert rep["cov_valid"] == (1 if rc == 0 else 0)
            if rc == 0:
                np.testing.assert_allclose(cov, cov_o, rtol=1e-7)
        # and the two entry points against each other (test_batch_matches_single_calls)
        np.testing.assert_allclose(work[i].theta, G.theta, rtol=0, atol=1e-8)
        np.testing.assert_allclose(covs[i], cov_s, rtol=1e-7)
    assert any(sum(r["iters"]) > 0 for r in reps)


# ------------------------------------------------------------------ judge
@functools.lru_cache(maxsize=None)
def judge_scene():
    """text_judge_planes at 1280 x 720, with detection centres added on the truncated corners of every true plane (the quad's boundary), on points of its edges,
    and at the image's last row and column"""
    w, h = MID
    with synth.camera(w, h, camera_K(w, h)):
        S = synth.text_judge_planes(seed=3, n=8)
    extra = []
    for i, kind in enumerate(S["kind"]):
        if kind != "true":
            continue
        u, v, _ = synth._judge_corners(S["theta"][i], S["Tcr"][i], S["box_ray"][i], S["K"])
        tu, tv = np.trunc(u), np.trunc(v)
        for b in range(4):
            extra.append((tu[b], tv[b]))                                                  # a corner: on the boundary lines
            extra.append((np.floor(0.5*(tu[b] + tu[(b + 1) % 4])), np.floor(0.5*(tv[b] + tv[(b + 1) % 4]))))      # near an edge's middle: on or next to the line
    extra += [(w - 1.0, 10.0), (10.0, h - 1.0), (w - 1.0, h - 1.0), (w - 1.4, h - 1.4), (w - 0.51, h - 0.51), (0.0, 0.0)]
    S["dete_xy"] = np.concatenate([S["dete_xy"], np.array(extra, np.float64)])
    return S


def test_judge_association_by_point_tests(oracle_lib):
    from textslam_amd.frame import Frame
    w, h = MID
    S = judge_scene()
    assert S["cur_img"].shape == (h, w)
    off, uv, inten = [0], [], []
    for q in S["quad"]:
        u, v, I, _ = oracle_lib.frame_box_pixels(S["ref_img"], q, 0.0, 1.0)
        uv.append(np.stack([u, v], 1)); inten.append(I.astype(np.uint8)); off.append(off[-1] + len(u))
    pix = (np.array(off, np.int32), np.concatenate(uv).astype(np.int16), np.concatenate(inten))
    fr = Frame(0); fr.GetPyrMat(S["cur_img"], 2)
    out = fr.TextJudgeBatch(0, S["theta"], S["Tcr"], S["box_ray"], pix[0], pix[1], pix[2], S["K"], S["K"], cos_min=0.0, out_margin=6, zncc_min=0.1, dete_xy=S["dete_xy"])
    reasons = _check_against_ref(out, S, pix, S["cur_img"], w0h0=(w, h))             # pass, reason, cos, zncc, box and every detection bit
    owned = [int(np.count_nonzero(out["dete"][k])) for k, r in enumerate(reasons) if r == PASS]
    print("reasons %s; detections owned by the passing planes %s" % (reasons, owned))
    assert PASS in reasons and max(owned) >= 1
    # level 1 against a level-0 association above the mask (the judge's image and the label image are different levels)
    K1 = S["K"]/2.0
    cur1 = oracle_lib.frame_pyramid(S["cur_img"], 2)[1][0]
    out1 = fr.TextJudgeBatch(1, S["theta"], S["Tcr"], S["box_ray"], pix[0], pix[1], pix[2], S["K"], K1, cos_min=0.0, out_margin=3, zncc_min=0.1, dete_xy=S["dete_xy"])
    _check_against_ref(out1, S, pix, cur1, K=K1, margin=3, w0h0=(w, h))


# ------------------------------------------------------------------ sizes in sequence, limit
def test_sizes_in_sequence_in_one_context(oracle_lib):
    """640 x 480, then 1280 x 720, then 640 x 480 again in ONE context: the first and the third result are the same bits (no buffer keeps the first call's size)"""
    from textslam_amd.optimizer import Optimizer
    g = Optimizer(0)
    o = abi.options_local()
    small, mid = synth.tiny(), tiny_at(*MID)
    runs = []
    for P in (small, mid, small):
        G = P.copy()
        rep = g.LocalBundleAdjustment(G, options=o)
        hh, ww = int(P.img[0].shape[1]), int(P.img[0].shape[2])
        lab = g.TextLabelImage(P.n_kf - 1, 0, (hh, ww))
        runs.append((G, rep, lab))
    g.close()
    key = lambda r: (r["iters"], r["accepted"], r["termination"], r["cost0"], r["cost1"], r["n_bad_scene"], r["n_bad_tfeat"], r["n_bad_text"])
    a, b = runs[0], runs[2]
    assert key(a[1]) == key(b[1])
    assert a[0].pose.tobytes() == b[0].pose.tobytes() and a[0].rho.tobytes() == b[0].rho.tobytes() and a[0].theta.tobytes() == b[0].theta.tobytes()
    assert np.array_equal(a[0].sgood, b[0].sgood) and np.array_equal(a[0].tobs_good, b[0].tobs_good) and np.array_equal(a[0].tfgood, b[0].tfgood)
    assert np.array_equal(a[2], b[2]) and (a[2] >= 0).any()
    R = mid.copy(); rep_o = oracle_lib.solve(R, o)
    assert runs[1][1]["iters"] == rep_o["iters"] and runs[1][1]["accepted"] == rep_o["accepted"]
    np.testing.assert_allclose(runs[1][0].pose, R.pose, rtol=0, atol=1e-8)
    assert np.array_equal(runs[1][2], oracle_lib.label_image(runs[1][0], mid.n_kf - 1, 0))


def test_limit_is_stated_and_named(gpu):
    """a level wider than TSBA_MAX_IMAGE_DIM: TSBA_ERR_ARG, and the error text names the limit"""
    import re
    from textslam_amd.optimizer import TsbaError
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define TSBA_MAX_IMAGE_DIM (\d+)", open(os.path.join(root, "include", "tsba.h")).read())
    assert m and int(m.group(1)) == 8192
    P = synth.tiny().copy()
    for l in range(P.n_levels):                                                         # the same problem over images one pixel too wide and a few rows high
        P.img[l] = np.zeros((P.n_kf, 8, (8192 >> l) + 1), np.uint8)
    with pytest.raises(TsbaError) as e:
        gpu.upload(P.normalise(), abi.options_local())
    assert "-1" in str(e.value) and "TSBA_MAX_IMAGE_DIM" in str(e.value), str(e.value)
    rep = gpu.LocalBundleAdjustment(tiny_at(648, 480).copy(), options=abi.options_local())     # the context is usable afterwards
    assert sum(rep["iters"]) > 0
