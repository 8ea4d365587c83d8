"""tsorb_match_two_view_reconstruct on the GPU: the two-view initializer's ReconstructH / ReconstructF in one call (include/tsorb.h,
textslam_amd/csrc/tstwoview_rec.h) against the numpy restatement (tests/two_view_reconstruct_ref.py, docs/twoview_reconstruct_recalled.md).  Per world:

  1. bit for bit, no conditions needed: from the device's OWN float hyp_pose and hyp_p3d the restatement's CheckRT arithmetic gives the device's hyp_state, hyp_good and
     hyp_cos as bit patterns, its keep logic gives result, and R21, t21, p3d and triangulated follow (hyp_parallax within 4 float steps: acosf is the platform's);
  2. hypotheses: every entry within the larger of 1000 x the restatement's sensitivity (inputs moved at the 1e-13 relative level in double) and one float ulp of the
     hypothesis' largest entry;
  3. points: every hyp_p3d point within the larger of 1000 x its own sensitivity and one float ulp of its largest coordinate (sensitivities measured 2e-13 ... 8e-10 on
     the committed worlds: the single float rounding is the floor);
  4. decisions: on the worlds that meet their conditions (asserted on the restatement alone by tests/test_two_view_reconstruct_ref.py) result, the kept hypothesis'
     triangulated mask and its hyp_good equal the restatement's outright, a non-kept hypothesis' hyp_good within +- its low-margin pairs.

n = 1, 8, 9, 63, 64, 65, 257, 300 matches, masks with 0 - 30 % zeros, both models, every exit; the call is a function of its arguments; a match's exit and point do not
depend on the other matches; every argument error with the outputs untouched; the resident frame and its grid undisturbed; the adapter from C++ byte for byte."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import two_view_reconstruct_ref as R                                  # noqa: E402
import two_view_reconstruct_io as IO                                  # noqa: E402

pytestmark = pytest.mark.gpu


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
    """Every world, the restatement's answer, its sensitivities, whether its conditions hold and its margins -- computed once, read-only."""
    out = {}
    for name in R.ALL:
        w, res = R.make(name), R.answer(name)
        out[name] = (w, res, R.sensitivity(w, res)) + R.conditions_hold(w, res)
    return out


def call(ex, w, **kw):
    g = lambda k: kw.get(k, w[k])
    return ex.match_two_view_reconstruct(g("xy1"), g("xy2"), g("inlier"), g("model"), g("M21"), g("K"), g("sigma"), g("min_parallax"), g("min_triangulated"))


@pytest.mark.parametrize("name", R.ALL)
def test_against_the_restatement(ex, worlds, name):
    w, ref, sens, holds, mg = worlds[name]
    got = call(ex, w)
    print("result", got["result"].tolist(), ref["result"].tolist(), "good", got["hyp_good"].tolist(), "parallax", got["hyp_parallax"].tolist(), "conditions hold:", holds)
    IO.check_bits(R, got, w)                                             # 1. bit for bit from the device's own hypotheses and points
    a = IO.check_hypotheses(R, got, ref, sens)                           # 2. the hypotheses
    b = IO.check_points(R, got, w, sens["point"])                        # 3. the points
    print("largest difference: hypotheses %.3g, points %.3g of the tolerance (sensitivities %.2e, %.2e); floats that differ: %d of the hypotheses, %d of %d coordinates" % (
        a, b, sens["pose"].max(), sens["point"].max(), int((IO.bits(got["hyp_pose"]) != IO.bits(ref["hyp_pose"])).sum()),
        int((IO.bits(got["hyp_p3d"]) != IO.bits(ref["hyp_p3d"])).sum()), ref["hyp_p3d"].size))
    assert holds, "a committed world does not meet its conditions"
    IO.check_decisions(R, got, ref, mg, w["model"])                      # 4. the decisions
    again = call(ex, w)                                                  # the call is a function of its arguments
    assert all(np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes() for k in got)


def test_a_match_does_not_depend_on_the_others(ex, worlds):
    """hyp_state and hyp_p3d of a match are the same bytes when the other matches are permuted or dropped: a lane turns its own matrix until IT has converged."""
    for name in ("h_tie_257", "f_drop_300"):
        w = worlds[name][0]; got = call(ex, w); n = w["n"]
        p = np.random.default_rng(5).permutation(n)
        q = call(ex, w, xy1=w["xy1"][p], xy2=w["xy2"][p], inlier=w["inlier"][p])
        assert q["hyp_state"].tobytes() == got["hyp_state"][:, p].tobytes() and q["hyp_p3d"].tobytes() == np.ascontiguousarray(got["hyp_p3d"][:, p]).tobytes()
        assert q["hyp_good"].tobytes() == got["hyp_good"].tobytes() and q["hyp_cos"].tobytes() == got["hyp_cos"].tobytes() and q["result"].tobytes() == got["result"].tobytes()
        for keep in (p[:70], p[:1], np.arange(3, n, 5)):
            q = call(ex, w, xy1=w["xy1"][keep], xy2=w["xy2"][keep], inlier=w["inlier"][keep])
            assert q["hyp_state"].tobytes() == np.ascontiguousarray(got["hyp_state"][:, keep]).tobytes()
            assert q["hyp_p3d"].tobytes() == np.ascontiguousarray(got["hyp_p3d"][:, keep]).tobytes() and q["hyp_pose"].tobytes() == got["hyp_pose"].tobytes()


def test_the_specific_cases(ex, worlds):
    w = worlds["identity"][0]; got = call(ex, w)                         # H's singular-value exit: nothing is evaluated
    assert got["result"].tolist() == [0, -1, 64, 0, 0, R.EXIT_SV] and not any(np.asarray(got[k]).any() for k in got if k.startswith("hyp_"))
    w = worlds["infinity"][0]; got = call(ex, w)                         # parallel rays: the isfinite exit, in every hypothesis
    assert (got["hyp_state"][:4, 0] == R.NONFINITE).all() and not np.isfinite(got["hyp_p3d"][0, 0]).all() and got["ok"] and not got["triangulated"][0]
    assert np.array_equal(got["hyp_pose"][0], np.array([[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32))
    w = worlds["f_few_300"][0]; got = call(ex, w)
    assert got["result"][5] == R.EXIT_FEW
    low = call(ex, w, min_triangulated=5, inlier=w["inlier"] & (got["hyp_state"][0] >= R.GOOD))       # the mask is the argument's: its good matches alone initialise
    assert low["ok"] and low["result"][2] == low["result"][3] == got["result"][3]
    wide = call(ex, w, sigma=3.0); IO.check_bits(R, wide, dict(w, sigma=np.float32(3.0)))             # sigma is the argument's
    assert wide["hyp_pose"].tobytes() == got["hyp_pose"].tobytes() and wide["hyp_good"][0] >= got["hyp_good"][0]
    w = worlds["f_success_65"][0]; got = call(ex, w)
    far = call(ex, w, min_parallax=30.0); IO.check_bits(R, far, dict(w, min_parallax=np.float32(30.0)))
    assert got["ok"] and far["result"][5] == R.EXIT_PARALLAX and far["hyp_good"].tobytes() == got["hyp_good"].tobytes()


# ------------------------------------------------------------------ argument errors
F32, I32, U8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
NAME = "tsorb_match_two_view_reconstruct"
_OUT = dict(result=(I32, -77), R21=(F32, 7.0), t21=(F32, 7.0), p3d=(F32, 7.0), triangulated=(U8, 0x5a), hyp_good=(I32, -77), hyp_cos=(F32, 7.0), hyp_parallax=(F32, 7.0),
            hyp_pose=(F32, 7.0), hyp_state=(U8, 0x5a), hyp_p3d=(F32, 7.0))


def _raw(ex, w, n=None, model=None, sigma=None, min_parallax=None, min_triangulated=None, null=(), ctx=True, mutate=None):
    a = dict(xy1=np.ascontiguousarray(w["xy1"], np.float32).copy(), xy2=np.ascontiguousarray(w["xy2"], np.float32).copy(), inlier=np.asarray(w["inlier"], np.uint8).copy(),
             M21=np.ascontiguousarray(w["M21"], np.float32).reshape(9).copy(), K=np.asarray(w["K"], np.float32).copy())
    if mutate:
        mutate(a)
    N = len(a["xy1"])
    shape = dict(result=6, R21=9, t21=3, p3d=(N, 3), triangulated=N, hyp_good=8, hyp_cos=8, hyp_parallax=8, hyp_pose=(8, 12), hyp_state=(8, N), hyp_p3d=(8, N, 3))
    o = {k: np.full(shape[k], v, {I32: np.int32, F32: np.float32, U8: np.uint8}[t]) for k, (t, v) in _OUT.items()}
    pi = lambda k, t: None if k in null else a[k].ctypes.data_as(t)
    po = lambda k: None if k in null else o[k].ctypes.data_as(_OUT[k][0])
    val = lambda x, k: float(w[k]) if x is None else x
    rc = ex.lib.tsorb_match_two_view_reconstruct(ex.ctx if ctx else None, N if n is None else n, pi("xy1", F32), pi("xy2", F32), pi("inlier", U8),
                                                 int(w["model"]) if model is None else model, pi("M21", F32), pi("K", F32), val(sigma, "sigma"), val(min_parallax, "min_parallax"),
                                                 int(w["min_triangulated"]) if min_triangulated is None else min_triangulated,
                                                 *[po(k) for k in _OUT])
    return rc, all(bool((o[k] == v).all()) for k, (_, v) in _OUT.items()), o


def test_arguments(ex, worlds):
    w = worlds["f_9"][0]
    ref = call(ex, w)

    def refused(named=True, **kw):
        rc, untouched, _ = _raw(ex, w, **kw)
        assert rc == -1 and untouched, kw
        if named:
            assert NAME in ex.lib.tsorb_last_error(ex.ctx).decode()

    refused(ctx=False, named=False)
    refused(n=0); refused(n=-1); refused(n=65537)
    refused(model=2); refused(model=-1)
    for k in ("xy1", "xy2", "inlier", "M21", "K", "result", "R21", "t21", "p3d", "triangulated"):
        refused(null=(k,))
    for key, idx in (("xy1", (8, 1)), ("xy2", (0, 0)), ("M21", (0,)), ("M21", (8,)), ("K", (0,)), ("K", (3,))):
        for badv in (np.nan, np.inf, -np.inf):
            def nf(a, key=key, idx=idx, badv=badv): a[key][idx] = badv
            refused(mutate=nf)
    for j in (0, 1):
        for badv in (0.0, -130.0):
            def nk(a, j=j, badv=badv): a["K"][j] = badv
            refused(mutate=nk)
    for s in (-1.0, float("nan"), float("inf")):
        refused(sigma=s); refused(min_parallax=s)
    refused(min_triangulated=-1)
    big = dict(w, xy1=np.ones((65537, 2), np.float32), xy2=np.ones((65537, 2), np.float32), inlier=np.ones(65537, bool))     # above TSORB_TWOVIEW_MAX_POINTS
    rc, untouched, _ = _raw(ex, big); assert rc == -1 and untouched
    # the optional outputs may be NULL, and the context still answers
    same = lambda o, keys: all(np.asarray(o[k]).reshape(-1).tobytes() == np.asarray(ref[k] if k != "triangulated" else ref[k].astype(np.uint8)).reshape(-1).tobytes() for k in keys)
    rc, untouched, o = _raw(ex, w)
    assert rc == 0 and not untouched and same(o, _OUT)
    hyp = tuple(k for k in _OUT if k.startswith("hyp_"))
    rc, _, o = _raw(ex, w, null=hyp)
    assert rc == 0 and same(o, [k for k in _OUT if k not in hyp]) and all((o[k] == _OUT[k][1]).all() for k in hyp)
    rc, _, o = _raw(ex, w, null=("hyp_p3d", "hyp_good"))
    assert rc == 0 and same(o, [k for k in _OUT if k not in ("hyp_p3d", "hyp_good")]) and (o["hyp_p3d"] == 7.0).all() and (o["hyp_good"] == -77).all()
    rc, _, o = _raw(ex, w, null=("hyp_state",))
    assert rc == 0 and same(o, [k for k in _OUT if k != "hyp_state"]) and (o["hyp_state"] == 0x5a).all()
    again = call(ex, w)
    assert all(np.asarray(again[k]).tobytes() == np.asarray(ref[k]).tobytes() for k in ref)


def test_resident_frame_not_disturbed(worlds):
    """A call between tsorb_match_set_frame and tsorb_match_search leaves the resident batch, the grid and the search results as they were."""
    from textslam_amd.orbextractor import ORBextractor, synthetic_frame
    w, ref, _, _, mg = worlds["h_success_64"]
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
    IO.check_bits(R, got, w); IO.check_decisions(R, got, ref, mg, w["model"])
    after = ex2.download()
    assert all(b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes() for b, a in zip(before, after))
    assert all(m0[k].tobytes() == m1[k].tobytes() for k in m0)


def test_adapter_from_cxx(tmp_path, ex, worlds):
    """adapter/tsorb_two_view.hpp's reconstruct over the driver's mock types: the gather and every output byte for byte the Python mirror's on the same arrays, vP3D and
    vbTriangulated scattered through .first; a reconstruction that fails returns false and leaves the matrices empty."""
    exe = IO.build_driver(tmp_path)
    for name in ("h_success_64", "f_drop_300", "h_tie_257", "f_1", "identity"):
        w = worlds[name][0]
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "two view reconstruct from C++: ok" in r.stdout, r.stdout + r.stderr
        o = IO.read_scene(outp, host=False)
        got = call(ex, w)
        assert o["result"].tolist() == got["result"].tolist() and o["R21"].tobytes() == got["R21"].tobytes() and o["t21"].tobytes() == got["t21"].tobytes()
        assert o["p3d"].tobytes() == got["p3d"].tobytes() and np.array_equal(o["triangulated"], got["triangulated"])
        IO.check_scene(o, w, got)
        assert bool(o["ret"]) == (name in ("h_success_64", "f_drop_300", "f_1"))
