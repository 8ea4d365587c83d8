"""The restatement of the two-view reconstruction (tests/two_view_reconstruct_ref.py, docs/twoview_reconstruct_recalled.md) on its own, and the device's
__host__ __device__ arithmetic on the CPU against it -- no GPU:

  * ground truth: on worlds that initialise the kept R21, t21 and the triangulated points are the true motion and the true points up to the scale of t;
  * a hand example: one match and a pure x-translation -- P2, the 4 x 4, the point, both errors and the cosine by hand;
  * the keep logic on hand-made counts, comparison for comparison;
  * every committed world meets its conditions, and the worlds take every exit, every size and both sides of the min(50, nGood - 1) branch;
  * tests/cxx/two_view_reconstruct_host.hip, built with the address and undefined-behaviour sanitizers, against the restatement on every world;
  * adapter/tsorb_two_view.hpp's reconstruct over mock types in --host mode."""
import math
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import two_view_reconstruct_ref as R                                  # noqa: E402
import two_view_reconstruct_io as IO                                  # noqa: E402

F32 = np.float32


def _angle(Ra, Rb):
    D = Ra.T @ Rb; s = 0.5*math.sqrt((D[2, 1] - D[1, 2])**2 + (D[0, 2] - D[2, 0])**2 + (D[1, 0] - D[0, 1])**2)      # the sine: an acos of the trace resolves 5e-4 rad in float
    return math.atan2(s, (np.trace(D) - 1.0)/2.0)


@pytest.mark.parametrize("name", ["h_success_64", "f_success_65", "f_63", "f_51", "f_drop_300"])
def test_ground_truth(name):
    """The kept pose is the true motion and the kept points are the true points, up to the scale of t (t21 has unit length, so X = X_true / |t_true|).

    Bounds, from the world's noise.  A pixel error of s px is a ray error of s/f rad (f = 130).  A model fitted to eight such matches and kept among 200 cannot be
    better than that, and its rotation error stays within 10 s/f: 0.038 rad for the RANSAC worlds (s = 0.5), and -- the model of a scene world is the true one
    rounded to float, a relative 6e-8 -- 1e-4 rad there.  The direction of t is seen through the parallax b/z (baseline over depth, 0.45/4 at the least on the RANSAC
    worlds), which divides the same ray error: 10 (s/f) (z/b) = 0.34 rad, and 1e-3 rad for the true models.  A triangulated depth moves by z (z/b) sqrt(2) s/f for a
    ray error in each view: with z/b <= 8/0.4 and s = 0.3 that is 6.5 % of the depth on the scene worlds, and every point is held to 5 times that, 33 %, the median to
    6.5 % itself.  (The RANSAC worlds do not keep their true points; the pose is what they check.)"""
    w = R.make(name); res = R.answer(name)
    assert res["result"][0] == 1
    ransac = R.WORLDS[name][0] is R.ransac_world
    rot = _angle(res["R21"].astype(np.float64), w["R"]); tt = w["t"]/np.linalg.norm(w["t"])
    tang = math.atan2(float(np.linalg.norm(np.cross(res["t21"].astype(np.float64), tt))), float(res["t21"].astype(np.float64) @ tt))
    print(name, "rotation error %.2e rad, translation direction error %.2e rad" % (rot, tang))
    assert rot <= (0.038 if ransac else 1e-4) and tang <= (0.34 if ransac else 1e-3)
    assert abs(np.linalg.det(res["R21"].astype(np.float64)) - 1.0) < 1e-5 and abs(np.linalg.norm(res["t21"]) - 1.0) < 1e-6
    if not ransac:
        tri = res["triangulated"]; Xt = w["X"][tri]/np.linalg.norm(w["t"])
        rel = np.linalg.norm(res["p3d"][tri] - Xt, axis=1)/np.linalg.norm(Xt, axis=1)
        print(name, "points: worst %.3f, median %.3f of the distance" % (rel.max(), np.median(rel)))
        assert tri.sum() >= 0.9*w["inlier"].sum() and rel.max() <= 0.33 and np.median(rel) <= 0.065


def test_hand_example():
    """K = (2, 2, 1, 1), R = I, t = (1, 0, 0), X = (2, -2, 4): the pixels are (2, 0) and (2.5, 0), every number below is a dyadic rational and exact in float."""
    K = np.array([2, 2, 1, 1], F32); iK = np.array([[.5, 0, -.5], [0, .5, -.5], [0, 0, 1.0]])
    Fm = iK.T @ R._skew([1.0, 0, 0]) @ iK                                # K^T F K = [t]x exactly
    w = dict(xy1=np.array([[2, 0]], F32), xy2=np.array([[2.5, 0]], F32), inlier=np.array([True]), model=1, M21=Fm.astype(F32), K=K, sigma=F32(1), min_parallax=F32(1),
             min_triangulated=0)
    assert np.array_equal(Fm.astype(F32).astype(np.float64), Fm)
    res = R.run(w)
    assert np.array_equal(res["hyp_pose"][0], np.array([[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0]], F32))              # R1 = I (the larger trace), t = +x (the sign rule)
    assert np.array_equal(res["hyp_pose"][2, :, 3], np.array([-1, 0, 0], F32)) and np.array_equal(res["hyp_pose"][1, :, :3], np.diag([1, -1, -1]).astype(F32))
    P2, O2 = R.camera(np.eye(3), [1, 0, 0], K)
    assert np.array_equal(P2, np.array([[2, 0, 1, 2], [0, 2, 1, 0], [0, 0, 1, 0]], F32)) and np.array_equal(O2, np.array([-1, 0, 0], F32))
    A = R.system(P2, K, w["xy1"], w["xy2"])[0]
    assert np.array_equal(A, np.array([[-2, 0, 1, 0], [0, -2, -1, 0], [-2, 0, 1.5, -2], [0, -2, -1, 0]], F32))
    assert np.array_equal(A @ np.array([2, -2, 4, 1], F32), np.zeros(4, F32))
    assert np.array_equal(res["hyp_p3d"][0, 0], np.array([2, -2, 4], F32))
    st, cs, q = R.check(np.eye(3), [1, 0, 0], K, R.th2_of(1.0), [True], w["xy1"], w["xy2"], res["hyp_p3d"][0])
    assert q["e1"][0] == 0 and q["e2"][0] == 0 and q["z1"][0] == 4 and q["z2"][0] == 4 and R.th2_of(1.0) == 4
    d1, d2 = F32(math.sqrt(24.0)), F32(math.sqrt(29.0))                   # |(2, -2, 4)| and |(3, -2, 4)|, double square roots rounded to float
    c = F32(26.0/np.float64(d1*d2))                                       # (2, -2, 4) . (3, -2, 4) = 26
    assert cs[0] == c and abs(float(c) - 26.0/math.sqrt(24.0*29.0)) < 1e-7 and st[0] == R.TRI
    # the four-fold ambiguity of E: the point is in front of both cameras in one hypothesis only, the other three leave at a depth test
    assert res["hyp_state"][0, 0] == R.TRI and all(s in (R.DEPTH1, R.DEPTH2) for s in res["hyp_state"][1:4, 0]) and not res["hyp_state"][4:].any()
    assert res["hyp_good"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and res["hyp_cos"][0] == c
    assert abs(float(res["hyp_parallax"][0]) - math.degrees(math.acos(26.0/math.sqrt(24.0*29.0)))) < 1e-4
    assert res["result"].tolist() == [1, 0, 1, 1, 1, 0] and np.array_equal(res["p3d"][0], np.array([2, -2, 4], F32)) and res["triangulated"][0]


def test_keep_logic():
    par = [5.0]*8
    # H: :787 -- secondBestGood < 0.75 bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 N
    assert R.keep(0, False, [10, 100, 74, 0, 0, 0, 0, 0], par, 100, 50, 1.0) == [1, 1, 100, 100, 74, 0]
    assert R.keep(0, False, [10, 100, 75, 0, 0, 0, 0, 0], par, 100, 50, 1.0) == [0, -1, 100, 100, 75, R.EXIT_TIE]             # 75 < 75.0 is false
    assert R.keep(0, False, [100, 100, 0, 0, 0, 0, 0, 0], par, 100, 50, 1.0) == [0, -1, 100, 100, 100, R.EXIT_TIE]            # the second of equal counts is second best
    assert R.keep(0, False, [0, 90, 0, 0, 0, 0, 0, 0], par, 100, 50, 1.0) == [0, -1, 100, 90, 0, R.EXIT_FEW]                  # 90 > 90.0 is false
    assert R.keep(0, False, [0, 50, 0, 0, 0, 0, 0, 0], par, 50, 50, 1.0) == [0, -1, 50, 50, 0, R.EXIT_FEW]                    # 50 > 50 is false
    assert R.keep(0, False, [0, 91, 0, 0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0, 0, 0], 100, 50, 1.0) == [1, 1, 100, 91, 0, 0]     # >= minParallax
    assert R.keep(0, False, [0, 91, 0, 0, 0, 0, 0, 0], [9, 0.99, 9, 9, 9, 9, 9, 9], 100, 50, 1.0) == [0, -1, 100, 91, 0, R.EXIT_PARALLAX]
    assert R.keep(0, False, [0]*8, par, 0, 0, 1.0) == [0, -1, 0, 0, 0, R.EXIT_TIE | R.EXIT_PARALLAX | R.EXIT_FEW]             # bestParallax stays -1
    assert R.keep(0, True, [0]*8, par, 64, 50, 1.0) == [0, -1, 64, 0, 0, R.EXIT_SV]
    # F: :560-633 -- nMinGood = max((int)(0.9 N), minTriangulated); > 0.7 maxGood counts itself; the else-if chain takes the FIRST of equal counts
    assert R.keep(1, False, [100, 70, 0, 0], par, 100, 50, 1.0) == [1, 0, 100, 100, 1, 0]                                     # 70 > 70.0 is false
    assert R.keep(1, False, [100, 71, 0, 0], par, 100, 50, 1.0) == [0, -1, 100, 100, 2, R.EXIT_TIE]
    assert R.keep(1, False, [0, 0, 89, 0], par, 100, 50, 1.0) == [0, -1, 100, 89, 1, R.EXIT_FEW]                              # (int)(90.0) = 90
    assert R.keep(1, False, [0, 0, 90, 0], par, 100, 50, 1.0) == [1, 2, 100, 90, 1, 0]
    assert R.keep(1, False, [0, 0, 90, 0], [9, 9, 1.0, 9], 100, 50, 1.0) == [0, -1, 100, 90, 1, R.EXIT_PARALLAX]              # > minParallax
    assert R.keep(1, False, [0, 40, 0, 0], par, 41, 5, 1.0) == [1, 1, 41, 40, 1, 0]                                           # (int)(36.9) = 36
    assert R.keep(1, False, [3, 3, 0, 0], par, 3, 0, 1.0) == [0, -1, 3, 3, 2, R.EXIT_TIE]


def test_order_statistic_and_parallax():
    g = np.random.default_rng(3); c = g.uniform(0.9, 1.0, 200).astype(F32); st = np.full(200, R.TRI, np.uint8); st[::3] = R.DEPTH1
    n, pick, par = R.statistic(st, c); kept = np.sort(c[st >= R.GOOD])
    assert n == len(kept) and pick == kept[50] and abs(float(par) - math.degrees(math.acos(float(pick)))) < 1e-4
    n, pick, _ = R.statistic(st[:60], c[:60]); kept = np.sort(c[:60][st[:60] >= R.GOOD])
    assert n == 40 and pick == kept[39]                                   # min(50, nGood - 1): the largest cosine
    assert R.statistic(np.zeros(5, np.uint8), c[:5]) == (0, 0, 0)


@pytest.fixture(scope="module")
def margins():
    return {name: R.conditions_hold(R.make(name), R.answer(name)) for name in R.ALL}


def test_every_committed_world_meets_the_conditions(margins):
    """The conditions of the decisions comparison, on the restatement alone, and the cases the worlds are there for."""
    taken, sizes, exits = set(), set(), set()
    for name in R.ALL:
        w, res = R.make(name), R.answer(name); holds, mg = margins[name]
        nh = 8 if w["model"] == 0 else 4; ev = np.maximum(mg["evaluated"][:nh], 1)
        print("%-15s n %3d N %3d result %s good %s low-margin pairs %s of %s (%.0f %% at most) parallax margins %s" % (
            name, w["n"], int(w["inlier"].sum()), res["result"].tolist(), res["hyp_good"][:nh].tolist(), mg["low"][:nh].tolist(), mg["evaluated"][:nh].tolist(),
            100.0*float((mg["low"][:nh]/ev).max()), np.round(np.minimum(mg["par_margin"][:nh], 1e9), 0).tolist()))
        assert holds, name + " does not meet its conditions"
        taken |= set(np.unique(res["hyp_state"]).tolist()); sizes.add(w["n"]); exits.add((w["model"], int(res["result"][5])))
    assert taken == set(range(8)), taken                                             # every exit a match can take
    assert (R.answer("f_err2_64")["hyp_state"][:4, 11] == R.ERR2).any()
    assert {1, 8, 9, 63, 64, 65, 257, 300} <= sizes
    assert {(0, 0), (1, 0), (0, R.EXIT_SV), (0, R.EXIT_TIE), (1, R.EXIT_FEW), (1, R.EXIT_PARALLAX)} <= exits and any(m == 0 and b & R.EXIT_PARALLAX for m, b in exits)
    kept = {name: int(R.answer(name)["result"][3]) for name in ("f_9", "f_51", "f_success_65")}
    assert kept["f_9"] < 51 and kept["f_51"] == 51 and kept["f_success_65"] > 51
    assert any((R.answer(n)["hyp_good"][:4] == 0).any() and R.answer(n)["result"][0] for n in R.ALL)                    # a hypothesis with nGood = 0 beside a kept one
    assert (R.answer("infinity")["hyp_state"][:4, 0] == R.NONFINITE).all() and not np.isfinite(R.answer("infinity")["hyp_p3d"][0, 0]).all()
    zeros = [1.0 - R.make(n)["inlier"].mean() for n in R.ALL]
    assert min(zeros) == 0.0 and 0.25 <= max(zeros) <= 0.4


def test_sensitivities_are_below_the_float_rounding():
    """The fp64 stages are defined by their inputs far below a float step: the single rounding is the floor of the device comparison."""
    worst = dict(pose=0.0, point=0.0)
    for name in R.ALL:
        s = R.sensitivity(R.make(name), R.answer(name)); worst = {k: max(worst[k], float(s[k].max())) for k in worst}
    print("largest sensitivity: hypotheses %.2e, points %.2e (a float step is 6e-8)" % (worst["pose"], worst["point"]))
    assert 1000.0*worst["pose"] < 6e-8 and 1000.0*worst["point"] < 6e-6


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return IO.build_host(str(tmp_path_factory.mktemp("rec_host") / "two_view_reconstruct_host"))


@pytest.mark.parametrize("name", R.ALL)
def test_host_program_under_sanitizers(host_exe, margins, tmp_path, name):
    """The device's own functions, compiled for the CPU with -fsanitize=address,undefined, give the restatement's answer: comparison 1 bit for bit, the hypotheses
    and the points within their tolerances, the decisions outright."""
    w, ref = R.make(name), R.answer(name)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    IO.write_host(inp, w)
    r = subprocess.run([host_exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "two view reconstruct host: ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    got = IO.read_host(outp, w["n"])
    IO.check_bits(R, got, w)
    sens = R.sensitivity(w, ref)
    a = IO.check_hypotheses(R, got, ref, sens); b = IO.check_points(R, got, w, sens["point"])
    print("largest difference: hypotheses %.3g, points %.3g of the tolerance; floats that differ: %d of the hypotheses, %d of %d coordinates" % (
        a, b, int((IO.bits(got["hyp_pose"]) != IO.bits(ref["hyp_pose"])).sum()), int((IO.bits(got["hyp_p3d"]) != IO.bits(ref["hyp_p3d"])).sum()), ref["hyp_p3d"].size))
    IO.check_decisions(R, got, ref, margins[name][1], w["model"])


def test_adapter_host_mode(tmp_path):
    """adapter/tsorb_two_view.hpp over the driver's mock types, no device: the gather, the floats of the model and of mK, and the reference's output types filled from
    given outputs -- vP3D / vbTriangulated sized like mvKeys1 and indexed through .first; a reconstruction that fails leaves everything as it was."""
    exe = IO.build_driver(tmp_path)
    for name in ("h_success_64", "f_drop_300", "h_tie_64", "f_1", "identity"):
        w, ref = R.make(name), R.answer(name)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w, ref)
        r = subprocess.run([exe, "--host", inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "two view reconstruct from C++ (host): ok" in r.stdout, r.stdout + r.stderr
        IO.check_scene(IO.read_scene(outp, host=True), w, ref)
