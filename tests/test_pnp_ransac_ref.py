"""The numpy restatement of CheckMatch's PnP RANSAC (tests/pnp_ransac_ref.py) against what it must be by construction, the conditions every committed world has to
meet, the host build of the device's __host__ __device__ arithmetic (textslam_amd/csrc/tspnp.h, as a stand-alone program under the host sanitizers) against the
restatement, and the adapter's driver in its --host mode.  No GPU."""
import math
import os
import struct
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ransac_ref as R                                            # noqa: E402
import pnp_check_io as IO                                             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worlds():
    out = {}
    for c in R.CASES + R.SPECIAL + ["degenerate"]:
        w = R.degenerate_world() if c == "degenerate" else R.world(*c)
        res = R.run_world(w)
        out[c] = (w, res, R.conditions(w, res))
    return out


# ------------------------------------------------------------------ the generator and the subsets
def test_cvrng_one_step_by_hand():
    """state = 2^64 - 1: low word 0xFFFFFFFF, carry 0xFFFFFFFF.  0xFFFFFFFF * 0xF83F630A (= 4164903690) = 0xF83F630A00000000 - 0xF83F630A = 0xF83F630907C09CF6;
    + 0xFFFFFFFF = 0xF83F630A07C09CF5."""
    g = R.CvRng()
    assert 4164903690 == 0xF83F630A
    assert g.next() == 0x07C09CF5 and g.state == 0xF83F630A07C09CF5
    g2 = R.CvRng(g.state)                                              # and the next step from that state, by the formula
    assert g2.next() == ((0x07C09CF5*4164903690 + 0xF83F630A) & 0xFFFFFFFF)
    assert R.CvRng().uniform(0, 300) == 0x07C09CF5 % 300


@pytest.mark.parametrize("n", [6, 7, 21, 300])
def test_subsets_distinct_and_in_range(n):
    s = R.draw_subsets(n, 100)
    assert s.shape == (100, 5) and s.min() >= 0 and s.max() < n
    assert all(len(set(row)) == 5 for row in s.tolist())
    assert np.array_equal(s, R.draw_subsets(n, 100))                   # a function of n alone
    assert np.array_equal(s[:7], R.draw_subsets(n, 7))
    if n == 6:                                                         # a repeated draw is drawn again, nothing else is skipped: replay the stream by hand
        g = R.CvRng(); seen = []
        while len(seen) < 5:
            v = g.next() % 6
            if v not in seen:
                seen.append(v)
        assert s[0].tolist() == seen


def test_five_matches_give_the_one_subset():
    assert R.draw_subsets(5, 100).tolist() == [[0, 1, 2, 3, 4]]


# ------------------------------------------------------------------ RANSACUpdateNumIters and the loop
def test_update_num_iters():
    assert R.update_num_iters(0.98, 0.0, 100) == 0                     # denom = 1 - 1 = 0 < DBL_MIN
    assert R.update_num_iters(0.98, 1.0, 100) == 100                   # denom = log(1) = 0 >= 0
    # by hand: log(0.02) = -3.912023, 1 - 0.7^5 = 0.83193, log = -0.184007, ratio 21.26 -> 21
    assert R.update_num_iters(0.98, 0.3, 100) == 21
    assert R.update_num_iters(0.98, 0.3, 20) == 20                     # -num >= max_iters * -denom: 3.912 >= 3.680
    assert R.update_num_iters(1.0, 0.3, 100) == 100                    # num = log(DBL_MIN) = -708.4: 708.4 >= 18.4
    assert R.cv_round(0.5) == 0 and R.cv_round(1.5) == 2 and R.cv_round(2.5) == 2


def test_walk():
    n = 100
    assert R.walk([50, 50, 50] + [0]*97, n)[:3] == (True, 50, 0)                 # the first of equal counts stays
    assert R.walk([4]*100, n) == (False, 0, -1, 100)                             # counts <= 4 are never kept
    assert R.walk([0, 5, 4, 3] + [0]*96, n)[:3] == (True, 5, 1)
    ok, good, sel, n_run = R.walk([0, 0, 70] + [99]*97, n)                       # ep = 0.3 after hypothesis 2: 21 iterations in all; hypothesis 3 (99) then cuts further
    assert (ok, good, sel) == (True, 99, 3) and n_run == 4                       # ep = 0.01: log(0.02) / log(1 - 0.99^5) = 1.3 -> 1 < 4 already run
    assert R.walk([0, 0, 70] + [0]*97, n) == (True, 70, 2, 21)                   # the early stop
    assert R.walk([100] + [0]*99, n) == (True, 100, 0, 1)                        # ep = 0: niters = 0


# ------------------------------------------------------------------ EPnP
def test_basis_rule_makes_the_pose_independent_of_the_null_basis(worlds):
    w = worlds[R.CASES[6]][0]
    Pw = w["Pw"].astype(np.float64); uv = w["uv"].astype(np.float64)
    worst = 0.0
    for s in w["subsets"][:40]:
        a = R.epnp5(Pw[s], uv[s], w["K"])
        for ang in (0.7, -2.1):
            worst = max(worst, float(np.abs(R.epnp5(Pw[s], uv[s], w["K"], rotate_null=ang) - a).max()))
    print("largest change of a pose under a rotation of v[0], v[1]: %.2e" % worst)
    assert worst <= 1e-10


def test_noise_free_data_return_the_pose(worlds):
    """Every hypothesis of the noise-free world returns the world's pose to what float-rounded inputs allow.  Measured: 1.14e-6 over the 100 hypotheses (the float
    rounding of points at depth 2 - 8 and of pixels up to 640, through five-point fits); asserted with a margin of 10."""
    w, res, _ = worlds[R.NOISE_FREE]
    d = float(np.abs(res["poses"] - w["pose"]).max())
    print("largest distance of a noise-free hypothesis from the pose: %.2e" % d)
    assert d <= 1.14e-5
    assert res["counts"] == [64]*100 and (res["ok"], res["n_inlier"], res["sel"], res["n_run"]) == (True, 64, 0, 1) and res["mask"].all()


def test_degenerate_subsets_are_results(worlds):
    w, res, _ = worlds["degenerate"]
    assert np.isnan(res["poses"][0]).all() and np.isnan(res["poses"][1]).all() and np.isfinite(res["poses"][2:]).all()
    assert res["counts"][:2] == [0, 0] and max(res["counts"]) > 4 and res["ok"] and res["sel"] >= 2


# ------------------------------------------------------------------ the committed worlds
def test_every_committed_world_meets_the_conditions(worlds):
    for c, (w, res, cond) in worlds.items():
        print(c, cond, (res["ok"], res["n_inlier"], res["sel"], res["n_run"]))
        assert cond["err_margin"] >= R.MIN_ERR_MARGIN, (c, cond)
        assert cond["gap"] >= R.MIN_GAP, (c, cond)
        assert cond["round_margin"] >= R.MIN_ROUND_MARGIN, (c, cond)


def test_the_worlds_cover_the_cases(worlds):
    for c in R.CASES[6:9]:                                             # the recipe at n = 300, 30 % outliers: the mask is the true inlier set, the walk stops early
        w, res, _ = worlds[c]
        assert np.array_equal(res["mask"], w["truth"]) and 20 <= res["n_run"] <= 25
    assert sorted(set(len(worlds[c][0]["subsets"]) for c in R.CASES)) == [1, 4, 5, 100, 128]
    assert sorted(set(c[1] for c in R.CASES)) == [5, 21, 64, 65, 256, 257, 300, 1000]
    w, res, _ = worlds[R.NO_CONSENSUS]
    assert not res["ok"] and res["sel"] == -1 and res["n_run"] == 100 and not res["mask"].any()
    w, res, _ = worlds[R.BEHIND]                                       # matches behind the camera are inliers: there is no test on the depth's sign
    X = w["Pw"][w["behind"]].astype(np.float64) @ w["pose"][:, :3].T + w["pose"][:, 3]
    assert len(w["behind"]) == 40 and (X[:, 2] < 0).all() and res["mask"][w["behind"]].all() and np.array_equal(res["mask"], w["truth"])


# ------------------------------------------------------------------ the device's arithmetic on the host
def _host_io(path, w):
    n, H = len(w["Pw"]), len(w["subsets"])
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", n, H)); f.write(w["K"].tobytes()); f.write(struct.pack("<dd", w["reproj_err"], w["confidence"]))
        f.write(w["Pw"].tobytes()); f.write(w["uv"].tobytes()); f.write(np.ascontiguousarray(w["subsets"], np.int32).tobytes())


def test_host_build_of_the_device_arithmetic(tmp_path, worlds):
    """textslam_amd/csrc/tspnp.h's __host__ __device__ functions in a stand-alone program with the host sanitizers (address, undefined), on the CPU: the decisions
    equal the restatement's, the poses within 1000 x the restatement's own sensitivity to a 1e-13 scaling of its inputs."""
    exe = str(tmp_path / "pnp_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "cxx", "pnp_host.hip")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")             # (the HIP runtime's own start-up allocations are not this program's)
    for c in (R.CASES[6], "degenerate"):
        w, res, _ = worlds[c]
        n, H = len(w["Pw"]), len(w["subsets"])
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        _host_io(inp, w)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "pnp host: ok" in r.stdout, r.stdout + r.stderr
        raw = open(outp, "rb").read()
        hp = np.frombuffer(raw, np.float64, 12*H, 0).reshape(H, 3, 4); hc = np.frombuffer(raw, np.int32, H, 96*H)
        r4 = np.frombuffer(raw, np.int32, 4, 100*H); inl = np.frombuffer(raw, np.uint8, n, 100*H + 16)
        tol = 1000.0*R.pose_sensitivity(w, res)
        assert np.array_equal(np.isnan(hp), np.isnan(res["poses"]))
        d = float(np.nanmax(np.abs(hp - res["poses"])))
        print(c, "host program against the restatement: %.2e (tolerance %.2e)" % (d, tol))
        assert d <= tol
        assert hc.tolist() == res["counts"] and r4.tolist() == [int(res["ok"]), res["n_inlier"], res["sel"], res["n_run"]]
        assert np.array_equal(inl.astype(bool), res["mask"])


# ------------------------------------------------------------------ the adapter without a device
def test_adapter_driver_on_the_host(tmp_path, worlds):
    exe = IO.build(tmp_path)
    for c, ok in ((R.CASES[1], True), (R.CASES[3], True), (R.CASES[0], False)):
        w, res, _ = worlds[c]
        s = IO.scene(w, seed=c[0])
        Pw, uv, K = IO.gather(s)
        assert np.abs(Pw - w["Pw"]).max() <= 1e-5                      # the scene is the world, up to the float of another route
        g = np.random.default_rng(c[1]); mask = (g.random(len(Pw)) < 0.6).astype(np.uint8)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write(inp, s, mask=mask, ok=ok)
        r = subprocess.run([exe, "--host", inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "pnp check from C++ (host): ok" in r.stdout, r.stdout + r.stderr
        o = IO.read(outp, len(s["match"]), host=True)
        assert o["n"] == len(Pw) and o["Pw"].tobytes() == Pw.tobytes() and o["uv"].tobytes() == uv.tobytes() and o["K"].tobytes() == K.tobytes()
        assert np.array_equal(o["subset"], R.draw_subsets(len(Pw), 100))
        want = s["match"].copy(); m = np.flatnonzero(want >= 0)
        want[m[(mask == 0) | (not ok)]] = -1
        assert np.array_equal(o["match"], want) and o["ret"] == int((want >= 0).sum()) == (int(mask.sum()) if ok else 0)
