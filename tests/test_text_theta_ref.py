"""The restatement of the new text planes' RANSAC (tests/text_theta_ref.py, docs/texttheta_recalled.md) on its own, and the device's __host__ __device__ arithmetic on
the CPU against it -- no GPU:

  * ground truth: the kept theta is the true plane within bounds derived from the world's noise;
  * a hand example in dyadic rationals: a pure x-translation, three features, every intermediate exact;
  * the vectorised restatement equals the scalar one in every bit; the selection on hand-made scores (ties, a NaN, all NaN);
  * every committed world's float points are unchanged under the sensitivity probe, and the worlds cover the sizes the kernels branch on;
  * tests/cxx/text_theta_host.hip, built with the address and undefined-behaviour sanitizers, bit-equal to the restatement on every world;
  * adapter/tsorb_text_theta.hpp's two bodies over mock types in --host mode against a plain transcription of the reference's loops, the draws included."""
import math
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_theta_ref as R                                            # noqa: E402
import text_theta_io as IO                                            # noqa: E402

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("name", ["n8_h64", "n63_h65", "n64_h200", "n65_h257", "n257_h200", "n1024_h64", "n20_h200", "n60_h200", "mixed_9", "batch_33"])
def test_ground_truth(name):
    """The kept plane predicts the true inverse depth of the features it counts, and it counts the plane's features.

    Bounds, from the world's noise.  A feature is counted when the plane's prediction lies within sqrt(5.991) = 2.45 px of its target.  A noise-only target lies
    within 5 sigma = 1.5 px of the true projection (sigma = 0.3 px per axis: a 2-D Gaussian exceeds 5 sigma with probability exp(-12.5) = 4e-6, the worlds have 6000
    features).  Prediction and true projection lie on the feature's epipolar line, where a relative change e of rho moves the projection by e x the feature's
    disparity (|projection - projection at infinity|, about f b/z = 458 x 0.25/3 = 38 px) to first order; t_z/z <= 0.1/3 and e <= 0.15 leave the second-order term
    below a quarter of that.  So for every counted noise-only feature |rhoPred/rho - 1| <= 1.25 (2.45 + 1.5)/disparity, about 13 %.
    The count: of 64 or more triples with 25 % outliers one is outlier-free except with probability (1 - 0.42)^64 = 1e-15, and the plane through three features
    whose depths are good to sigma/disparity = 0.8 % reprojects the plane's other features within the 2.45 px; the kept hypothesis has the largest score, so it is
    held to counting at least half of the noise-only features (planes of 8 or more features and 64 or more hypotheses)."""
    w = R.make(name); res = R.answer(name); T = np.asarray(w["Tcr"], F64).reshape(12); K = [float(v) for v in w["K"]]
    for p in range(len(w["off"]) - 1):
        a, b, nh = int(w["off"][p]), int(w["off"][p + 1]), int(w["hyp_off"][p + 1] - w["hyp_off"][p])
        if b - a < 8 or nh < 64:
            continue
        assert res["sel"][p] >= 0
        th = -res["theta"][p]; F = R.features(w, res["rho"])[a:b]
        chi = R.chi_of(T, K, th, F.T); counted = chi <= R.TH; inl = w["inlier"][a:b]
        m = np.column_stack([F[:, 0], F[:, 1], np.ones(b - a)]); rho_true = m @ w["truth"][p]; pred = m @ th
        rel = np.abs(pred/rho_true - 1.0); bound = 1.25*(math.sqrt(R.TH) + 1.5)/w["disparity"][a:b]
        k = counted & inl
        print("%s plane %d: n %d, noise-only %d, counted %d of them (and %d others), worst |rhoPred/rho - 1| %.4f of a bound of %.4f" % (
            name, p, b - a, int(inl.sum()), int(k.sum()), int((counted & ~inl).sum()), float(rel[k].max()) if k.any() else 0.0, float(bound[k].min()) if k.any() else 0.0))
        assert (rel[k] <= bound[k]).all()
        assert k.sum() >= 0.5*inl.sum()


def _hand():
    """K = (2, 2, 1, 1), Tcr = [I | (1, 0, 0)], the plane z = 4 (rho = 0.25): rays (0, 0.5), (0.5, 0), (1, 1) -> host pixels (1, 2), (2, 1), (3, 3), points (0, 2, 4),
    (2, 0, 4), (4, 4, 4), targets (1.5, 2), (2.5, 1), (3.5, 3)."""
    return dict(off=np.array([0, 3], np.int32), hyp_off=np.array([0, 1], np.int32), host_xy=np.array([[1, 2], [2, 1], [3, 3]], F32),
                targ_xy=np.array([[1.5, 2], [2.5, 1], [3.5, 3]], F32), triple=np.array([[0, 1, 2]], np.int32), Tcr=np.array([[1, 0, 0, 1.0], [0, 1, 0, 0], [0, 0, 1, 0]]),
                K=np.array([2.0, 2, 1, 1]), rho=np.array([0.25, 0.25, 0.25]))


def test_hand_example():
    w = _hand(); F = R.features(w, w["rho"])
    assert np.array_equal(F, np.array([[0, .5, .25, 1.5, 2], [.5, 0, .25, 2.5, 1], [1, 1, .25, 3.5, 3]]))
    # A = 1, B = 1, C = (1 - 0.5)/(0 - 0.5) = -1, D = (-2 x 0) + 0.5 + 1 = 1.5, rho3' = 0.25, rho2' = 0.125/-0.5 = -0.25, rho1' = 0.25 + 0.25 x 0.5 = 0.375
    th = R.solve(F[0], F[1], F[2])
    assert [float(x) for x in th] == [0.0, 0.0, 0.25]                    # theta3 = 0.375/1.5, theta2 = -0.25 + 0.25, theta1 = 0.25 - 0 - 0.25
    T = w["Tcr"].reshape(12)
    for f in F:                                                           # rhoPred = 0.25, P = 4 (m0, m1, 1) + (1, 0, 0), u = P0/4 x 2 + 1: the targets exactly
        assert R.chi_of(T, w["K"], th, f) == 0.0
    res = R.run(w)
    assert res["sel"].tolist() == [0] and res["score"][0] == (R.TH + R.TH) + R.TH and R.TH == float(F32(5.991)) and R.TH != 5.991
    assert res["theta"][0].tolist() == [0.0, 0.0, -0.25] and np.signbit(res["theta"][0]).all()          # the negated theta: -0.0, -0.0, -0.25
    assert not res["p3d"].any() and np.array_equal(res["rho"], w["rho"])
    # the same example through the triangulation: the 4 x 4 rows by hand, (0, 2, 4, 1) in its null space exactly; the float point after the SVD within one float step
    tri = dict(w, rho=None); A = R.system(tri)
    assert np.array_equal(A[0], np.array([[-1, 0, 0, 0], [0, -1, .5, 0], [-1, 0, .25, -1], [0, -1, .5, 0]]))
    assert not (A[0] @ np.array([0, 2, 4, 1.0])).any() and not (A[2] @ np.array([4, 4, 4, 1.0])).any()
    X, rho = R.triangulate(tri)
    assert (np.abs(X.astype(F64) - np.array([[0, 2, 4], [2, 0, 4], [4, 4, 4.0]])) <= np.spacing(F32(4))).all() and R.same64(rho, 1.0/X[:, 2].astype(F64))
    # Mat /= scalar as recalled: the reciprocal rounded to float, then a float product
    v = np.array([[5.0, -7.0, 10.0, 3.0]]); Y, r = R.points_of(v); third = F32(1.0/3.0)
    assert Y[0].tolist() == [float(F32(5)*third), float(F32(-7)*third), float(F32(10)*third)] and r[0] == 1.0/float(Y[0, 2])
    assert Y[0, 0] != F32(5)/F32(3) and Y[0, 0] != F32(5*(1.0/3.0))       # neither a float division nor a scale applied in double: the probe of the docs
    assert R.same32(R.points_of(-v)[0], Y)                                # the null vector's sign does not matter


def test_scalar_and_vector_restatements_agree():
    """`hypotheses` (numpy over a plane's hypotheses) is `hypothesis_scalar` (Python floats, one hypothesis) in every bit, degenerate triples included."""
    w = R.make("n20_h200"); F = R.features(w, R.answer("n20_h200")["rho"]).copy(); F[7, 0] = 0.0          # a feature at x == cx
    tri = np.vstack([w["triple"][:20], [[1, 2, 7], [7, 1, 2], [0, 0, 0], [3, 3, 4]]])
    hs, ht = R.hypotheses(w["Tcr"].reshape(12), w["K"], F, tri)
    for h, t in enumerate(tri):
        s, th = R.hypothesis_scalar(w["Tcr"].reshape(12).tolist(), [float(v) for v in w["K"]], F.tolist(), [int(x) for x in t])
        assert R.same64(np.array([s] + th), np.concatenate([[hs[h]], ht[h]])), (h, s, th, hs[h], ht[h])
    assert np.isnan(hs[20]) and np.isnan(ht[20]).all() and np.isfinite(ht[21]).all()


def test_selection():
    nan = float("nan")
    assert R.select([1.0, 3.0, 3.0, 2.0]) == 1                           # the first of equal largest scores
    assert R.select([nan, 2.0, nan, 2.0]) == 1 and R.select([5.0, nan]) == 0
    assert R.select([nan, nan, nan]) == -1 and R.select([]) == -1
    assert R.select([0.0, 0.0]) == 0 and R.select([-0.0]) == 0           # -1.0 < 0.0: a plane of outliers only keeps hypothesis 0
    assert R.select([-1.0, -2.0]) == -1                                  # (a score is never negative; the loop would not keep it)


def test_worlds_meet_the_condition_and_cover_the_shapes():
    sizes, hyps, planes = set(), set(), set()
    for name in R.ALL:
        w = R.make(name); s = R.sensitivity(w)
        print("%-10s planes %2d features %4d hypotheses %4d: sensitivity %.2e, float points moved by the probe: %d" % (
            name, len(w["off"]) - 1, int(w["off"][-1]), int(w["hyp_off"][-1]), float(s["rel"].max()), int((s["ulp"] > 0).sum())))
        assert R.conditions_hold(w), name
        assert 1000.0*float(s["rel"].max()) < 6e-8                       # the fp64 stage is defined far below a float step
        sizes |= set(np.diff(w["off"]).tolist()); hyps |= set(np.diff(w["hyp_off"]).tolist()); planes.add(len(w["off"]) - 1)
    assert {2, 3, 8, 63, 64, 65, 257, 1024} <= sizes and {0, 1, 64, 65, 200, 257} <= hyps and {1, 9, 33} <= planes
    w = R.make("mixed_9"); res = R.answer("mixed_9")
    assert res["sel"][2] == -1 and res["sel"][5] == -1 and (np.delete(res["sel"], [2, 5]) >= 0).all()                  # two features; no hypotheses
    assert 0.2 <= 1.0 - R.make("n1024_h64")["inlier"].mean() <= 0.3


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return IO.build_host(str(tmp_path_factory.mktemp("tt_host") / "text_theta_host"))


@pytest.mark.parametrize("name", R.ALL + R.GIVEN)
def test_host_program_under_sanitizers(host_exe, tmp_path, name):
    """The device's own functions, compiled for the CPU with -fsanitize=address,undefined, give the restatement's answer in every bit: the Jacobi null vector rounds
    to the float np.linalg.svd's rounds to on every committed world."""
    w = R.make(name); ref = R.answer(name) if name in R.ALL else R.run(w)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    IO.write_host(inp, w)
    r = subprocess.run([host_exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "text theta host: ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    got = IO.read_host(outp, w)
    IO.check_bits(R, got, w)
    if w.get("rho") is None:
        IO.check_points(R, got, w, R.sensitivity(w))
    assert R.same32(got["p3d"], ref["p3d"]) and R.same_answer(got, ref)


def test_host_program_on_degenerate_triples(host_exe, tmp_path):
    """x == cx in the third place, the same feature first, a repeated index, a collinear triple, outliers only, every hypothesis NaN: the same bits as the restatement."""
    w = R.make("n20_h200"); host = w["host_xy"].copy(); host[7, 0] = F32(w["K"][2]); host[0, 1] = host[1, 1] = host[2, 1]
    tri = w["triple"].copy(); tri[0] = (1, 2, 7); tri[1] = (7, 1, 2); tri[2] = (0, 0, 0); tri[3] = (0, 1, 2)
    allnan = tri.copy(); allnan[:, 0] = 1; allnan[:, 1] = 2; allnan[:, 2] = 7
    for d, sel in ((dict(w, host_xy=host, triple=tri), None), (dict(w, targ_xy=w["targ_xy"] + F32(500)), 0), (dict(w, host_xy=host, triple=allnan), -1)):
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_host(inp, d)
        r = subprocess.run([host_exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
        got = IO.read_host(outp, d); ref = R.run(d)
        IO.check_bits(R, got, d)
        assert R.same_answer(got, ref)
        if sel is None:
            assert np.isnan(got["hyp_score"][0]) and np.isfinite(got["hyp_theta"][1]).all() and got["sel"][0] > 0
        else:
            assert got["sel"].tolist() == [sel] and (np.isnan(got["hyp_score"]).all() if sel < 0 else not got["hyp_score"].any())


def test_adapter_host_mode(tmp_path):
    """adapter/tsorb_text_theta.hpp over the driver's mock types, no device: the driver itself holds mNcr / vNGOOD to a plain transcription of the reference's loops
    (its own draws from the same seed); here the gather, the draws and the scatter are held to the reference's rules and the restatement on the gathered batch."""
    exe = IO.build_driver(tmp_path)
    for name, mode in (("mixed_9", "track"), ("batch_33", "track"), ("init_9", "init")):
        w = R.make(name); rho = R.answer(name)["rho"] if mode == "track" else w["rho"]
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w, mode, rho)
        r = subprocess.run([exe, "--host", inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "text theta from C++ (host): ok" in r.stdout, r.stdout + r.stderr
        o = IO.read_scene(outp); d = IO.scene_call(w, mode, o)
        IO.check_scene(o, w, mode, d, R.run(d, rho=o["rho"]))
        if mode == "init":
            assert o["sel"][2] == -1 and o["sel"][7] == -1 and not o["triple"][o["hyp_off"][7]:o["hyp_off"][8]].any() and o["hyp_off"][3] == o["hyp_off"][2]
