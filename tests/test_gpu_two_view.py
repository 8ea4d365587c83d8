"""tsorb_match_two_view_ransac on the GPU: the two-view initializer's H / F RANSAC in one call (include/tsorb.h, textslam_amd/csrc/tstwoview.h) against the numpy
restatement (tests/two_view_ref.py, docs/twoview_recalled.md).

  * scoring, bit for bit, no conditions needed: the restatement's scoring of the device's OWN float models gives the device's hyp_score as bit patterns (NaNs in the
    same places), its keep loop gives the device's sel, and score, H21, F21 and both masks are what it derives from the kept models;
  * models: every hyp_model entry within the larger of 1000 x the restatement's sensitivity to a (1 + 1e-13) scaling of A and one float ulp of the matrix's largest
    entry (the single rounding can fall either way at a boundary); degenerate hypotheses NaN in both;
  * decisions: on the worlds whose conditions hold (tests/two_view_ref.py: conditions_hold) sel, both masks and RH's side of 0.40 equal the restatement's outright;
  * n = 8 (the one subset 0 .. 7), 9, 64, 65, 257, 300 matches and 1, 3, 200, 256 hypotheses; a planar and a general scene, 30 % outliers, a subset that is exactly
    rank-deficient for F, a world where every hypothesis is degenerate; every argument error with the outputs untouched; the resident frame and its grid undisturbed;
    the adapter from C++ byte for byte."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import two_view_ref as R                                              # noqa: E402
import two_view_io as IO                                              # noqa: E402

pytestmark = pytest.mark.gpu
_id = lambda c: c if isinstance(c, str) else "%s_seed%d_n%d_out%g_h%d" % c


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
    """Every world, the restatement's answer, its sensitivity and whether its conditions hold -- computed once, read-only."""
    out = {}
    for c in R.ALL:
        w = R.make(c); res = R.run_world(w)
        out[c] = (w, res, R.model_sensitivity(w, res), R.conditions_hold(w, res)[0])
    return out


def call(ex, w, **kw):
    return ex.match_two_view_ransac(w["xy1"], w["xy2"], w["norm1"], w["norm2"], kw.get("subsets", w["subsets"]), kw.get("sigma", w["sigma"]))


@pytest.mark.parametrize("case", R.ALL, ids=_id)
def test_against_the_restatement(ex, worlds, case):
    w, ref, sens, holds = worlds[case]
    got = call(ex, w)
    print("sel", got["sel"], ref["sel"], "score", got["score"], ref["score"], "RH", R.RH(got), R.RH(ref), "conditions hold:", holds)
    IO.check_scoring(R, got, w)                                          # 1. bit for bit from the device's own models
    worst = IO.check_models(R, got, ref, sens)                           # 2. the models
    print("largest model difference: %.3g of the tolerance (sensitivity %.2e); floats that differ: %d of %d"
          % (worst, sens, int((IO.bits(got["hyp_model"]) != IO.bits(ref["hyp_model"]))[~np.isnan(ref["hyp_model"])].sum()), ref["hyp_model"].size))
    assert holds, "a committed world does not meet its conditions"
    IO.check_decisions(R, got, ref)                                      # 3. the decisions
    again = call(ex, w)                                                  # the call is a function of its arguments
    assert all(np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes() for k in got)


def test_the_specific_cases(ex, worlds):
    w, ref, _, _ = worlds["twice"]; got = call(ex, w)                    # an exactly rank-deficient F subset: a NaN model and a NaN score, never kept; H is fine
    assert np.isnan(got["hyp_model"][1, 0]).all() and np.isnan(got["hyp_score"][1, 0]) and np.isfinite(got["hyp_model"][0]).all() and got["sel"][1] > 0
    w, ref, _, _ = worlds["same"]; got = call(ex, w)                     # every hypothesis degenerate: nothing kept
    assert np.isnan(got["hyp_model"]).all() and np.isnan(got["hyp_score"]).all() and got["sel"].tolist() == [-1, -1]
    assert not got["inlier_h"].any() and not got["inlier_f"].any() and not got["H21"].any() and not got["F21"].any() and got["score"].tolist() == [0.0, 0.0]
    w, ref, _, _ = worlds[R.PLANAR]; got = call(ex, w)
    assert R.RH(got) > 0.40
    w, ref, _, _ = worlds[R.OUTLIERS]; got = call(ex, w)
    assert R.RH(got) < 0.40 and (got["inlier_f"] & ~w["truth"]).sum() <= 0.1*len(w["truth"]) and got["inlier_f"][w["truth"]].mean() > 0.8
    few = call(ex, w, subsets=w["subsets"][:3])                          # the first hypotheses alone give the first hypotheses' models and scores
    assert few["hyp_model"].tobytes() == got["hyp_model"][:, :3].tobytes() and few["hyp_score"].tobytes() == got["hyp_score"][:, :3].tobytes()
    wide = call(ex, w, sigma=2.0); IO.check_scoring(R, wide, dict(w, sigma=2.0))     # sigma is the argument's
    assert wide["hyp_model"].tobytes() == got["hyp_model"].tobytes() and wide["inlier_f"].sum() > got["inlier_f"].sum()


# ------------------------------------------------------------------ argument errors
F32, I32, U8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
NAME = "tsorb_match_two_view_ransac"


def _raw(ex, w, n=None, n_hyp=None, sigma=1.0, null=(), ctx=True, mutate=None):
    a = dict(xy1=w["xy1"].copy(), xy2=w["xy2"].copy(), norm1=w["norm1"].copy(), norm2=w["norm2"].copy(), subset=np.ascontiguousarray(w["subsets"], np.int32).copy())
    if mutate:
        mutate(a)
    N, H = len(a["xy1"]), len(a["subset"])
    o = dict(inlier_h=np.full(N, 0x5a, np.uint8), inlier_f=np.full(N, 0x5a, np.uint8), H21=np.full(9, 7.0, np.float32), F21=np.full(9, 7.0, np.float32),
             score=np.full(2, 7.0, np.float32), sel=np.full(2, -77, np.int32), hyp_score=np.full((2, H), 7.0, np.float32), hyp_model=np.full((2, H, 9), 7.0, np.float32))
    p = lambda d, k, t: None if k in null else d[k].ctypes.data_as(t)
    rc = ex.lib.tsorb_match_two_view_ransac(ex.ctx if ctx else None, N if n is None else n, p(a, "xy1", F32), p(a, "xy2", F32), p(a, "norm1", F32), p(a, "norm2", F32),
                                            H if n_hyp is None else n_hyp, p(a, "subset", I32), sigma, p(o, "inlier_h", U8), p(o, "inlier_f", U8), p(o, "H21", F32),
                                            p(o, "F21", F32), p(o, "score", F32), p(o, "sel", I32), p(o, "hyp_score", F32), p(o, "hyp_model", F32))
    same = dict(inlier_h=0x5a, inlier_f=0x5a, H21=7.0, F21=7.0, score=7.0, sel=-77, hyp_score=7.0, hyp_model=7.0)
    return rc, all(bool((o[k] == v).all()) for k, v in same.items()), o


def test_arguments(ex, worlds):
    w = worlds[R.CASES[1]][0]                                            # 9 matches, 3 hypotheses
    ref = call(ex, w)

    def refused(named=True, **kw):
        rc, untouched, _ = _raw(ex, w, **kw)
        assert rc == -1 and untouched, kw
        if named:
            assert NAME in ex.lib.tsorb_last_error(ex.ctx).decode()

    refused(ctx=False, named=False)
    refused(n=7); refused(n=0); refused(n=-1); refused(n=65537)
    refused(n_hyp=0); refused(n_hyp=-3); refused(n_hyp=257)
    for k in ("xy1", "xy2", "norm1", "norm2", "subset", "inlier_h", "inlier_f", "H21", "F21", "score", "sel"):
        refused(null=(k,))

    def sub(i, j, v):
        def m(a): a["subset"][i, j] = v
        return m
    refused(mutate=sub(2, 3, 9)); refused(mutate=sub(0, 0, -1)); refused(mutate=sub(1, 7, 1 << 30))
    def twice(a): a["subset"][1, 6] = a["subset"][1, 2]
    refused(mutate=twice)
    for key, idx in (("xy1", (7, 1)), ("xy2", (0, 0)), ("norm1", (0,)), ("norm1", (3,)), ("norm2", (1,)), ("norm2", (2,))):
        for badv in (np.nan, np.inf, -np.inf):
            def nf(a, key=key, idx=idx, badv=badv): a[key][idx] = badv
            refused(mutate=nf)
    for key in ("norm1", "norm2"):
        for j in (2, 3):
            for badv in (0.0, -1.0):
                def ns(a, key=key, j=j, badv=badv): a[key][j] = badv
                refused(mutate=ns)
    for s in (0.0, -1.0, float("nan"), float("inf")):
        refused(sigma=s)
    big = dict(w, xy1=np.ones((65537, 2), np.float32), xy2=np.ones((65537, 2), np.float32))                      # above TSORB_TWOVIEW_MAX_POINTS
    rc, untouched, _ = _raw(ex, big); assert rc == -1 and untouched
    many = dict(w, subsets=np.tile(w["subsets"][:1], (257, 1)))
    rc, untouched, _ = _raw(ex, many); assert rc == -1 and untouched
    # the limit itself is legal, the optional outputs may be NULL, and the context still answers
    rc, untouched, o = _raw(ex, dict(w, subsets=np.tile(w["subsets"], (86, 1))[:256]))
    assert rc == 0 and not untouched and o["hyp_score"][:, :3].tobytes() == ref["hyp_score"].tobytes() and o["sel"].tolist() == ref["sel"].tolist()
    rc, _, o = _raw(ex, w, null=("hyp_score", "hyp_model"))
    assert rc == 0 and o["sel"].tolist() == ref["sel"].tolist() and o["score"].tobytes() == ref["score"].tobytes() and o["H21"].tobytes() == ref["H21"].tobytes()
    assert o["F21"].tobytes() == ref["F21"].tobytes() and np.array_equal(o["inlier_h"].astype(bool), ref["inlier_h"]) and np.array_equal(o["inlier_f"].astype(bool), ref["inlier_f"])
    assert (o["hyp_score"] == 7.0).all() and (o["hyp_model"] == 7.0).all()
    again = call(ex, w)
    assert all(np.asarray(again[k]).tobytes() == np.asarray(ref[k]).tobytes() for k in ref)


def test_resident_frame_not_disturbed(worlds):
    """A call between tsorb_match_set_frame and tsorb_match_search leaves the resident batch, the grid and the search results as they were."""
    from textslam_amd.orbextractor import ORBextractor, synthetic_frame
    w, ref, _, _ = worlds[R.PLANAR]
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
    IO.check_scoring(R, got, w); IO.check_decisions(R, got, ref)
    after = ex2.download()
    assert all(b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes() for b, a in zip(before, after))
    assert all(m0[k].tobytes() == m1[k].tobytes() for k in m0)


def test_adapter_from_cxx(tmp_path, ex, worlds):
    """adapter/tsorb_two_view.hpp over the driver's mock types: Normalize's statistics, the gather and every output byte for byte the Python mirror's on the same
    arrays; a world where nothing is kept returns false and leaves the matrices empty."""
    exe = IO.build_driver(tmp_path)
    for c in (R.PLANAR, R.OUTLIERS, "twice", "same"):
        w = worlds[c][0]
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "two view from C++: ok" in r.stdout, r.stdout + r.stderr
        o = IO.read_scene(outp, host=False)
        assert o["norm1"].tobytes() == w["norm1"].tobytes() and o["norm2"].tobytes() == w["norm2"].tobytes()
        assert o["xy1"].tobytes() == w["xy1"].tobytes() and o["xy2"].tobytes() == w["xy2"].tobytes() and np.array_equal(o["subset"], w["subsets"])
        got = call(ex, w)
        kept = got["sel"] >= 0
        assert o["sel"].tolist() == got["sel"].tolist() and o["ret"] == int(kept.all()) and (o["hasH"], o["hasF"]) == (int(kept[0]), int(kept[1]))
        assert np.array([o["SH"], o["SF"]], np.float32).tobytes() == got["score"].tobytes()
        assert o["H"].tobytes() == got["H21"].tobytes() and o["F"].tobytes() == got["F21"].tobytes()
        assert np.array_equal(o["inlH"], got["inlier_h"]) and np.array_equal(o["inlF"], got["inlier_f"])
        assert kept.all() == (c != "same")
