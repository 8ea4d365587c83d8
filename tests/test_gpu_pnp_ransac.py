"""tsorb_match_pnp_ransac on the GPU: tracking::CheckMatch's PnP RANSAC in one call (include/tsorb.h, textslam_amd/csrc/tspnp.h) against the numpy restatement
(tests/pnp_ransac_ref.py).

  * decisions are exact: every hypothesis' inlier count, n_run, sel, ok, n_inlier and the mask equal the restatement's as integers;
  * poses: hyp_pose and pose within a tolerance that comes from the restatement alone -- 1000 x the largest change of any hypothesis' R, t when the
    restatement's 3-D inputs are scaled by (1 + 1e-13), measured per world (1e-13 .. 5e-10, docs/pnpransac_recalled.md);
  * the worlds are held to conditions first (no error within 1e-2 px^2 of the threshold, eigenvalue gaps >= 1e-3 relative, no rounded iteration count within 1e-6
    of a half-integer): with them every integer above is decided by a margin far above that tolerance;
  * sizes 5, 21, 64 / 65, 256 / 257, 300, 1000 and 1, 4, 5, 100, 128 hypotheses; noise-free data, an early stop, no consensus, degenerate subsets, matches behind
    the camera, every argument error with the outputs untouched, a call between tsorb_match_set_frame and tsorb_match_search, the adapter from C++ byte for byte."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ransac_ref as R                                            # noqa: E402
import pnp_check_io as IO                                             # noqa: E402

pytestmark = pytest.mark.gpu
ALL = R.CASES + R.SPECIAL + ["degenerate"]
_id = lambda c: c if isinstance(c, str) else "seed%d_n%d_out%g_noise%g_h%d_behind%d" % c


@pytest.fixture(autouse=True)
def time_limit():
    """Each test under its own limit: a call that does not return ends the process with a traceback instead of holding the device."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ex():
    from textslam_amd.orbextractor import ORBextractor
    return ORBextractor()


@pytest.fixture(scope="module")
def worlds():
    """Every world, the restatement's answer, its conditions and the pose tolerance -- computed once, read-only."""
    out = {}
    for c in ALL:
        w = R.degenerate_world() if c == "degenerate" else R.world(*c)
        res = R.run_world(w); cond = R.conditions(w, res)
        assert cond["err_margin"] >= R.MIN_ERR_MARGIN and cond["gap"] >= R.MIN_GAP and cond["round_margin"] >= R.MIN_ROUND_MARGIN, (c, cond)
        out[c] = (w, res, 1000.0*R.pose_sensitivity(w, res))
    return out


def call(ex, w, **kw):
    return ex.match_pnp_ransac(w["Pw"], w["uv"], w["K"], w["subsets"], kw.get("reproj_err", w["reproj_err"]), kw.get("confidence", w["confidence"]))


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_against_the_restatement(ex, worlds, case):
    w, ref, tol = worlds[case]
    got = call(ex, w)
    print("counts", got["hyp_count"].tolist()[:12], "ref", ref["counts"][:12], "result", (got["ok"], got["n_inlier"], got["sel"], got["n_run"]),
          (ref["ok"], ref["n_inlier"], ref["sel"], ref["n_run"]))
    assert got["hyp_count"].tolist() == ref["counts"]
    assert (got["ok"], got["n_inlier"], got["sel"], got["n_run"]) == (ref["ok"], ref["n_inlier"], ref["sel"], ref["n_run"])
    assert got["inlier"].dtype == bool and np.array_equal(got["inlier"], ref["mask"])
    assert np.array_equal(np.isnan(got["hyp_pose"]), np.isnan(ref["poses"]))
    d = float(np.nanmax(np.abs(got["hyp_pose"] - ref["poses"])))
    print("largest pose difference %.2e, tolerance %.2e" % (d, tol))
    assert d <= tol
    if ref["ok"]:
        assert got["pose"].tobytes() == got["hyp_pose"][got["sel"]].tobytes() and got["n_inlier"] == int(got["inlier"].sum()) == got["hyp_count"][got["sel"]]
    else:
        assert not got["inlier"].any() and not got["pose"].any()
    again = call(ex, w)                                                # the call is a function of its arguments
    assert all(np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes() for k in got)


def test_the_specific_cases(ex, worlds):
    w, ref, _ = worlds[R.NOISE_FREE]; got = call(ex, w)
    assert got["hyp_count"].tolist() == [64]*100 and got["n_run"] == 1 and got["sel"] == 0 and got["inlier"].all()
    w, ref, _ = worlds[R.CASES[6]]; got = call(ex, w)                   # an early stop: 21 of 100, and still every hypothesis is reported
    assert got["n_run"] == 21 and len(got["hyp_count"]) == 100 and (got["hyp_count"][21:] > 4).any()
    w, ref, _ = worlds[R.NO_CONSENSUS]; got = call(ex, w)
    assert not got["ok"] and got["sel"] == -1 and got["n_inlier"] == 0 and got["n_run"] == 100 and not got["inlier"].any()
    w, ref, _ = worlds["degenerate"]; got = call(ex, w)
    assert np.isnan(got["hyp_pose"][:2]).all() and got["hyp_count"][:2].tolist() == [0, 0] and got["ok"] and got["sel"] >= 2 and np.isfinite(got["pose"]).all()
    only = dict(w, subsets=w["subsets"][:2]); got = call(ex, only)     # nothing but degenerate subsets: the call returns, nothing is kept
    assert not got["ok"] and got["hyp_count"].tolist() == [0, 0] and not got["inlier"].any() and got["n_run"] == 2
    w, ref, _ = worlds[R.BEHIND]; got = call(ex, w)
    assert got["inlier"][w["behind"]].all() and np.array_equal(got["inlier"], w["truth"])
    w, ref, _ = worlds[R.CASES[6]]                                      # the threshold and the confidence are the arguments'
    tight = call(ex, w, reproj_err=0.25)
    assert (tight["hyp_count"] <= np.array(ref["counts"])).all() and 4 < tight["n_inlier"] < ref["n_inlier"]
    assert call(ex, w, confidence=0.0)["n_run"] == R.run(w["Pw"], w["uv"], w["K"], w["subsets"], 5.0, 0.0)["n_run"] < 21 < call(ex, w, confidence=1.0)["n_run"] == 100


# ------------------------------------------------------------------ argument errors
F32, F64, I32, U8 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _raw(ex, w, n=None, n_hyp=None, reproj=5.0, conf=0.98, null=(), ctx=True, mutate=None):
    a = dict(Pw=w["Pw"].copy(), uv=w["uv"].copy(), K=w["K"].copy(), subset=np.ascontiguousarray(w["subsets"], np.int32).copy())
    if mutate:
        mutate(a)
    n = len(a["Pw"]) if n is None else n; H = len(a["subset"]) if n_hyp is None else n_hyp
    o = dict(inlier=np.full(len(a["Pw"]), 0x5a, np.uint8), result=np.full(4, -77, np.int32), pose=np.full(12, 7.0), hyp_count=np.full(len(a["subset"]), -77, np.int32),
             hyp_pose=np.full((len(a["subset"]), 12), 7.0))
    p = lambda d, k, t: None if k in null else d[k].ctypes.data_as(t)
    rc = ex.lib.tsorb_match_pnp_ransac(ex.ctx if ctx else None, n, p(a, "Pw", F32), p(a, "uv", F32), p(a, "K", F64), H, p(a, "subset", I32), reproj, conf,
                                       p(o, "inlier", U8), p(o, "result", I32), p(o, "pose", F64), p(o, "hyp_count", I32), p(o, "hyp_pose", F64))
    untouched = bool((o["inlier"] == 0x5a).all() and (o["result"] == -77).all() and (o["pose"] == 7.0).all() and (o["hyp_count"] == -77).all() and (o["hyp_pose"] == 7.0).all())
    return rc, untouched, o


def test_arguments(ex, worlds):
    w = worlds[R.CASES[2]][0]                                           # 64 matches, 5 hypotheses
    ref = call(ex, w)

    def refused(named=True, **kw):
        rc, untouched, _ = _raw(ex, w, **kw)
        assert rc == -1 and untouched, kw
        if named:
            assert "tsorb_match_pnp_ransac" in ex.lib.tsorb_last_error(ex.ctx).decode()

    refused(ctx=False, named=False)
    refused(n=4); refused(n=0); refused(n=-1)
    refused(n_hyp=0); refused(n_hyp=-3); refused(n_hyp=129)
    for k in ("Pw", "uv", "K", "subset", "inlier", "result"):
        refused(null=(k,))

    def sub(i, j, v):
        def m(a): a["subset"][i, j] = v
        return m
    refused(mutate=sub(2, 3, 64)); refused(mutate=sub(0, 0, -1)); refused(mutate=sub(4, 4, 1 << 30))
    def twice(a): a["subset"][3, 4] = a["subset"][3, 1]
    refused(mutate=twice)
    for key, idx in (("Pw", (7, 2)), ("uv", (63, 0)), ("K", (1,))):
        for badv in (np.nan, np.inf, -np.inf):
            def nf(a, key=key, idx=idx, badv=badv): a[key][idx] = badv
            refused(mutate=nf)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        refused(reproj=r)
    for cf in (-0.01, 1.01, float("nan")):
        refused(conf=cf)
    big = dict(Pw=np.ones((65537, 3), np.float32), uv=np.ones((65537, 2), np.float32), K=w["K"], subsets=w["subsets"])      # above TSORB_PNP_MAX_POINTS
    rc, untouched, _ = _raw(ex, big); assert rc == -1 and untouched
    many = dict(w, subsets=R.draw_subsets(64, 129))
    rc, untouched, _ = _raw(ex, many); assert rc == -1 and untouched
    # the limits themselves are legal, the optional outputs may be NULL, and the context still answers
    rc, untouched, o = _raw(ex, dict(w, subsets=R.draw_subsets(64, 128))); assert rc == 0 and not untouched and o["hyp_count"][:5].tolist() == ref["hyp_count"].tolist()
    rc, _, o = _raw(ex, w, null=("pose", "hyp_count", "hyp_pose"))
    assert rc == 0 and o["result"].tolist() == [int(ref["ok"]), ref["n_inlier"], ref["sel"], ref["n_run"]] and np.array_equal(o["inlier"].astype(bool), ref["inlier"])
    assert (o["pose"] == 7.0).all() and (o["hyp_count"] == -77).all() and (o["hyp_pose"] == 7.0).all()
    rc, _, o = _raw(ex, w, conf=0.0); assert rc == 0
    rc, _, o = _raw(ex, w, conf=1.0); assert rc == 0


def test_between_set_frame_and_search(worlds):
    """A call between tsorb_match_set_frame and tsorb_match_search leaves the resident batch, the grid and the search results as they were."""
    from textslam_amd.orbextractor import ORBextractor, synthetic_frame
    w, ref, _ = worlds[R.CASES[6]]
    ex2 = ORBextractor()
    ex2.extract_batch(np.stack([synthetic_frame(2, 320, 240), synthetic_frame(3, 320, 240)]))
    rng = np.random.default_rng(11)
    before = ex2.download()
    q = rng.choice(len(before[1][0]), 40, replace=False)
    args = (before[1][0][q, :2] + rng.uniform(-3, 3, (40, 2)).astype(np.float32), np.full(40, 12.0, np.float32), None, before[1][1][q])
    ex2.match_set_frame(1, (0.0, 320.0, 0.0, 240.0))
    m0 = ex2.match_search(*args)
    assert (m0["cand_cnt"] > 0).any()
    ex2.match_set_frame(1, (0.0, 320.0, 0.0, 240.0))
    got = call(ex2, w)
    m1 = ex2.match_search(*args)
    assert got["hyp_count"].tolist() == ref["counts"] and np.array_equal(got["inlier"], ref["mask"])
    after = ex2.download()
    assert all(b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes() for b, a in zip(before, after))
    assert all(m0[k].tobytes() == m1[k].tobytes() for k in m0)


def test_adapter_from_cxx(tmp_path, ex, worlds):
    """adapter/tsorb_pnp_check.hpp over the driver's mock types: the gather, the subsets and every output byte for byte the Python mirror's on the same arrays;
    fewer than five matches leave the matches alone and say so."""
    exe = IO.build(tmp_path)
    for c in (R.CASES[6], R.NO_CONSENSUS, R.CASES[0]):
        w = worlds[c][0]
        s = IO.scene(w, seed=c[0])
        Pw, uv, K = IO.gather(s)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write(inp, s)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "pnp check from C++: ok" in r.stdout, r.stdout + r.stderr
        o = IO.read(outp, len(s["match"]), host=False)
        assert o["called"] == 1 and o["Pw"].tobytes() == Pw.tobytes() and o["uv"].tobytes() == uv.tobytes() and o["K"].tobytes() == K.tobytes()
        subsets = R.draw_subsets(len(Pw), 100)
        assert np.array_equal(o["subset"], subsets)
        got = ex.match_pnp_ransac(Pw, uv, K, subsets, float(s["reproj"]), 0.98)
        assert o["result"].tolist() == [int(got["ok"]), got["n_inlier"], got["sel"], got["n_run"]] and o["pose"].tobytes() == got["pose"].tobytes()
        assert o["hyp_count"].tobytes() == got["hyp_count"].tobytes() and np.array_equal(o["inlier"].astype(bool), got["inlier"])
        want = s["match"].copy(); m = np.flatnonzero(want >= 0); want[m[~got["inlier"]]] = -1
        assert np.array_equal(o["match"], want) and o["ret"] == (got["n_inlier"] if got["ok"] else 0)
        assert got["ok"] == (c != R.NO_CONSENSUS)
    few = IO.scene(dict(worlds[R.CASES[1]][0]), seed=9)
    keep = np.flatnonzero(few["match"] >= 0)[4:]; few["match"][keep] = -1          # four matches are left
    IO.write(inp, few)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    o = IO.read(outp, len(few["match"]), host=False)
    assert o["called"] == 0 and o["ret"] == -1 and o["n"] == 4 and np.array_equal(o["match"], few["match"])
