"""The numpy restatement of the two-view initializer's H / F RANSAC (tests/two_view_ref.py) against ground truth and hand-computed examples, the conditions every
committed world has to meet, the host build of the device's __host__ __device__ arithmetic (textslam_amd/csrc/tstwoview.h, as a stand-alone program under the host
sanitizers) against the restatement, and the adapter's driver in its --host mode.  No GPU."""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import two_view_ref as R                                              # noqa: E402
import two_view_io as IO                                              # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def worlds():
    out = {}
    for c in R.ALL:
        w = R.make(c); res = R.run_world(w)
        out[c] = (w, res)
    return out


# ------------------------------------------------------------------ against ground truth
def test_planar_world_keeps_a_homography(worlds):
    """The kept H maps the inlier points of frame 1 onto frame 2 to within the noise (0.5 px a coordinate in both frames, through an eight-point fit: every kept
    inlier has chi^2 <= 5.991 in both directions by construction; the difference of two points with 0.5 px noise a coordinate has sigma 0.71 px a coordinate and a
    median length of 0.83 px, so with the error of an eight-point model on top the median transfer error is held under 1.5 px), and RH > 0.40."""
    w, res = worlds[R.PLANAR]
    H = res["H21"].astype(np.float64)
    x1 = np.column_stack([w["xy1"].astype(np.float64), np.ones(w["n"])]); y = x1 @ H.T; y = y[:, :2]/y[:, 2:]
    err = np.linalg.norm(y - w["xy2"], axis=1)[res["inlier_h"]]
    print("kept H: %d of %d inliers, transfer error median %.2f max %.2f px, RH %.3f" % (res["inlier_h"].sum(), w["n"], np.median(err), err.max(), R.RH(res)))
    assert res["inlier_h"].sum() >= 0.75*w["n"] and np.median(err) < 1.5 and err.max() <= np.sqrt(5.991) + 1e-3
    assert R.RH(res) > 0.40
    for c in R.CASES:
        if c[0] == "planar":
            assert R.RH(worlds[c][1]) > 0.40, c


def test_general_world_keeps_a_fundamental_matrix(worlds):
    """The kept F has x2^T F x1 small on its inliers (the epipolar distance, not the raw form: under sqrt(3.841) px by construction; the noise of both points
    across the line has sigma 0.71 px and a median magnitude of 0.48 px, so with the error of an eight-point model on top the median is held under 1 px), rank 2
    (third singular value below 1e-6 of the first: F21 = T2^T Fn T1 of an exactly rank-2 Fn, rounded to float), and RH < 0.40."""
    for c in (R.GENERAL, R.OUTLIERS):
        w, res = worlds[c]
        F = res["F21"].astype(np.float64)
        x1 = np.column_stack([w["xy1"].astype(np.float64), np.ones(w["n"])]); x2 = np.column_stack([w["xy2"].astype(np.float64), np.ones(w["n"])])
        l2 = x1 @ F.T; d = np.abs(np.sum(l2*x2, axis=1))/np.hypot(l2[:, 0], l2[:, 1])
        s = np.linalg.svd(F, compute_uv=False)
        print(c, "kept F: %d inliers, epipolar distance median %.2f max %.2f px, singular values %s, RH %.3f" % (res["inlier_f"].sum(), np.median(d[res["inlier_f"]]), d[res["inlier_f"]].max(), s, R.RH(res)))
        assert np.median(d[res["inlier_f"]]) < 1.0 and d[res["inlier_f"]].max() <= np.sqrt(3.841) + 1e-3
        assert s[2] <= 1e-6*s[0] and s[1] > 1e-3*s[0]
        assert R.RH(res) < 0.40
        assert (res["inlier_f"] & ~w["truth"]).sum() <= 0.1*w["n"] and res["inlier_f"][w["truth"]].mean() > 0.8


# ------------------------------------------------------------------ by hand
def test_scoring_two_matches_by_hand():
    """H21 = a shift by (2, 0), sigma = 1: H12 shifts back.  Match A: (10, 20) -> (12, 21): both transfer errors are (0, 1), chi^2 = 1, terms 5.991 - 1 twice.
    Match B: (30, 40) -> (35, 40): errors (3, 0), chi^2 = 9 > 5.991: no term, not an inlier.  Score = (0 + 4.991) + 4.991 in float.
    F21 = [[0, 0, 0], [0, 0, -1], [0, 1, 0]] (pure x translation: l2 = (0, -1, v1), distance |v2 - v1|).  A: chi^2 = 1 <= 3.841, terms 5.991 - 1 twice;
    a match with |v2 - v1| = 2 has chi^2 = 4 > 3.841: no term although 4 < 5.991."""
    xy1 = np.array([[10, 20], [30, 40]], F32); xy2 = np.array([[12, 21], [35, 40]], F32)
    H = np.array([[1, 0, 2], [0, 1, 0], [0, 0, 1]], F32)
    assert np.array_equal(R.h_inverse(H), np.array([[1, 0, -2], [0, 1, 0], [0, 0, 1]], F32))
    s, m = R.score(0, H, xy1, xy2)
    t = F32(F32(5.991) - F32(1))
    assert s == F32(F32(F32(0) + t) + t) and m.tolist() == [True, False]
    assert R.score_scalar(0, H, xy1, xy2)[0] == s
    Fm = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F32)
    xy2f = np.array([[12, 21], [35, 42]], F32)
    c1, c2, t1, t2, inl = R.terms(1, Fm, xy1, xy2f)
    assert c1.tolist() == [1.0, 4.0] and c2.tolist() == [1.0, 4.0] and inl.tolist() == [True, False] and t1.tolist() == [float(t), 0.0]
    s, m = R.score(1, Fm, xy1, xy2f)
    assert s == F32(t + t) and R.score_scalar(1, Fm, xy1, xy2f)[0] == s
    assert R.score(0, H, xy1, xy2, sigma=2.0)[1].tolist() == [True, True]        # chi^2 = 9 / 4
    assert R.h_inverse(np.zeros((3, 3), F32)).tolist() == np.zeros((3, 3)).tolist()   # a zero determinant gives zeros
    assert np.isnan(R.score(0, np.full((3, 3), np.nan, F32), xy1, xy2)[0])          # a NaN model scores NaN, which the keep loop never keeps
    assert R.keep([np.nan, 3.0, 3.0, np.nan, 2.0]) == (1, F32(3.0)) and R.keep([np.nan, 0.0]) == (-1, F32(0))


def test_vector_scoring_equals_the_scalar_loop(worlds):
    w, res = worlds[R.CASES[1]]
    for m in range(2):
        for h in range(3):
            a, ma = R.score(m, res["hyp_model"][m, h], w["xy1"], w["xy2"]); b, mb = R.score_scalar(m, res["hyp_model"][m, h], w["xy1"], w["xy2"])
            assert IO.same_floats(a, b) and np.array_equal(ma, mb)


def test_normalize_five_points_by_hand():
    """x = 1, 2, 3, 4, 10: mean 4, deviations 3, 2, 1, 0, 6: mean 2.4 (float), sX = float(1 / 2.4f).  y = 0, 0, 0, 0, 5: mean 1, deviations 1, 1, 1, 1, 4: mean
    1.6 (float).  T = [[sX, 0, -4 sX], [0, sY, -sY], [0, 0, 1]]; the point (10, 5) normalises to (6 sX, 4 sY)."""
    keys = np.array([[1, 0], [2, 0], [3, 0], [4, 0], [10, 5]], F32)
    n = R.normalize(keys)
    sX, sY = F32(1.0/np.float64(F32(12)/F32(5))), F32(1.0/np.float64(F32(8)/F32(5)))
    assert n.tolist() == [4.0, 1.0, float(sX), float(sY)]
    T = R.T_of(n)
    assert T.tolist() == [[float(sX), 0.0, float(F32(-4)*sX)], [0.0, float(sY), float(F32(-1)*sY)], [0.0, 0.0, 1.0]]
    assert R.normalized(keys[4:], n).tolist() == [[float(F32(6)*sX), float(F32(4)*sY)]]


def test_sign_rule_and_degenerate_subsets(worlds):
    assert R.sign_rule(np.array([0.1, -0.5, 0.5])).tolist() == [-0.1, 0.5, -0.5]       # the first of equal magnitudes decides
    w, res = worlds["twice"]
    assert np.isnan(res["hyp_model"][1, 0]).all() and np.isnan(res["hyp_score"][1, 0]) and np.isfinite(res["hyp_model"][0]).all() and res["sel"][1] > 0
    assert res["ratio"][1, 0] <= 1e-20 and res["ratio"][0, 0] >= R.MIN_RATIO
    w, res = worlds["same"]
    assert np.isnan(res["hyp_model"]).all() and res["sel"].tolist() == [-1, -1] and not res["inlier_h"].any() and not res["H21"].any() and res["score"].tolist() == [0, 0]


# ------------------------------------------------------------------ the committed worlds
def test_every_committed_world_meets_the_conditions(worlds):
    """Asserted on the restatement alone: every gap and margin at least 10 times the comparison's tolerance (what one float step of every entry of a model does to
    a score or a chi square, two_view_ref.decision_margins), every non-degenerate eigenvalue ratio at least 1e-6."""
    for c, (w, res) in worlds.items():
        holds, cond, over = R.conditions_hold(w, res, factor=10.0)
        print(c, cond, "in units of the tolerance:", over, "sensitivity %.2e" % R.model_sensitivity(w, res))
        assert over["gap"] >= 10.0 and over["margin"] >= 10.0, (c, over)
        assert cond["ratio"] >= 1e-6, (c, cond)
        assert holds
        assert R.model_sensitivity(w, res) <= 1e-10                    # 1000 x this stays below a float ulp (6e-8): the single rounding is the comparison's floor


def test_the_worlds_cover_the_cases(worlds):
    assert sorted(set(worlds[c][0]["n"] for c in R.CASES)) == [8, 9, 64, 65, 257, 300]
    assert sorted(set(len(worlds[c][0]["subsets"]) for c in R.CASES)) == [1, 3, 200, 256]
    assert worlds[R.CASES[0]][0]["subsets"].tolist() == [list(range(8))]
    assert {c[0] for c in R.CASES} == {"planar", "general"} and R.OUTLIERS[3] == 0.3
    for c in R.ALL:
        s = worlds[c][0]["subsets"]
        assert all(len(set(r)) == 8 for r in s.tolist()) and s.min() >= 0 and s.max() < worlds[c][0]["n"]


# ------------------------------------------------------------------ the device's arithmetic on the host
def test_host_build_of_the_device_arithmetic(tmp_path, worlds):
    """textslam_amd/csrc/tstwoview.h's __host__ __device__ functions in a stand-alone program with the host sanitizers (address, undefined), on the CPU, every world:
    the scoring bit for bit from the program's own float models, the models within the larger of 1000 x the restatement's sensitivity and one float ulp of the
    matrix's largest entry, the decisions equal to the restatement's."""
    exe = IO.build_host(str(tmp_path / "two_view_host"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")             # (the HIP runtime's own start-up allocations are not this program's)
    for c, (w, res) in worlds.items():
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_host(inp, w)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "two view host: ok" in r.stdout, r.stdout + r.stderr
        got = IO.read_host(outp, w["n"], len(w["subsets"]))
        IO.check_scoring(R, got, w)
        worst = IO.check_models(R, got, res, R.model_sensitivity(w, res))
        print(c, "host program against the restatement: %.3g of the tolerance" % worst)
        IO.check_decisions(R, got, res)


# ------------------------------------------------------------------ the adapter without a device
def test_adapter_driver_on_the_host(tmp_path, worlds):
    """two_view_normalize bit-equal to the restatement's, the gather, and the reference's output types filled from given outputs (a kept pair, and nothing kept)."""
    exe = IO.build_driver(tmp_path)
    for c in (R.PLANAR, R.CASES[1], "same"):
        w, res = worlds[c]
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w, given=res)
        r = subprocess.run([exe, "--host", inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "two view from C++ (host): ok" in r.stdout, r.stdout + r.stderr
        o = IO.read_scene(outp, host=True)
        assert o["norm1"].tobytes() == R.normalize(w["keys1"]).tobytes() and o["norm2"].tobytes() == R.normalize(w["keys2"]).tobytes()
        assert o["n"] == w["n"] and o["xy1"].tobytes() == w["keys1"][w["matches"][:, 0]].tobytes() and o["xy2"].tobytes() == w["keys2"][w["matches"][:, 1]].tobytes()
        assert np.array_equal(o["subset"], w["subsets"])
        kept = res["sel"] >= 0
        assert o["ret"] == int(kept.all()) and (o["hasH"], o["hasF"]) == (int(kept[0]), int(kept[1]))
        assert np.array([o["SH"], o["SF"]], F32).tobytes() == res["score"].tobytes() and o["H"].tobytes() == res["H21"].tobytes() and o["F"].tobytes() == res["F21"].tobytes()
        assert np.array_equal(o["inlH"], res["inlier_h"]) and np.array_equal(o["inlF"], res["inlier_f"])
